"""GPU: the host mirror's doc vectors (DeviceIndex.SetDocVectors / VectorSearch / RerankByVector through pybind) on the config-1 corpus
of test_gpu_host.py, against the model (tests/vector_model.py) by docHash.  Dense ids are the mirror's own, so among rows of equal score
any doc of that score is right; the engine's calls are compared byte for byte in test_gpu_vector.py."""
import numpy as np
import pytest

from tests import vector_model as vm
from tests.test_gpu_host import _weighted_tables, corpus, h, host  # noqa: F401  (module fixtures of the host-mirror test)

pytestmark = pytest.mark.gpu

DIM = 64


def test_vector_search_and_rerank_follow_the_model(host, corpus):
    forw, inv = _weighted_tables(host, corpus)
    doc = corpus["doc"]
    di = host.DeviceIndex()
    di.load(forw, inv)
    rng = np.random.default_rng(41)
    qvec = rng.integers(-128, 128, (4, DIM)).astype(np.int8)
    with pytest.raises(RuntimeError, match="SetDocVectors"):
        di.VectorSearch(qvec.tolist(), 5)
    with pytest.raises(RuntimeError, match="SetDocVectors"):
        di.RerankByVector(qvec.tolist(), [[]] * 4)
    # a vector for the first 900 pages, none (the zero vector) for the rest; a hash the index does not hold is ignored
    named = 900
    vec = rng.integers(-128, 128, (named, DIM)).astype(np.int8)
    vec[7] = vec[3]                                            # twins: a tie the dense ids break
    vectors = {doc[i]: vec[i].tolist() for i in range(named)}
    di.SetDocVectors({**vectors, h("http://nowhere/"): [1] * DIM})
    with pytest.raises(RuntimeError, match="length"):
        di.SetDocVectors({doc[0]: [1] * 65})
    score = vm.scores(qvec, vec)                               # [4][900]; every other doc scores 0
    at = {d: i for i, d in enumerate(doc[:named])}

    def check_all():
        for k in (1, 10, 50):
            rows = di.VectorSearch(qvec.tolist(), k)
            for q in range(4):
                got = [(r.DocHash, r.Score) for r in rows[q]]
                # the model's scores in order; a row's doc is one of the docs of that score (equal scores: the mirror's ids decide)
                want = sorted((int(score[q, i]) for i in range(named)), reverse=True)[:k]
                assert want[-1] > 0                             # (no doc without a vector, score 0, among the first 50)
                assert [s for _, s in got] == want, (q, k)
                assert len({d for d, _ in got}) == k
                for d, s in got:
                    assert d in vectors and int(score[q, at[d]]) == s
        # a mask: only pages 100 .. 199
        di.SetDocMasks({"some": [doc[i] for i in range(100, 200)]})
        rows = di.VectorSearch(qvec.tolist(), 20, ["some", "", "some", ""])
        for q in (0, 2):
            want = sorted(((doc[i], int(score[q, i])) for i in range(100, 200)), key=lambda x: -x[1])[:20]
            assert [r.Score for r in rows[q]] == [s for _, s in want]
            assert {r.DocHash for r in rows[q]} <= {doc[i] for i in range(100, 200)}
        assert rows[1][0].Score == int(score[1].max())
        # re-rank the lexical windows of four queries
        queries = ["w3 w40 w149", "w120", 'w7 "w1 w2"', "w0"]
        windows = di.RetrieveBatch(queries, 60)
        value = lambda r, q: int(score[q, at[r.DocHash]]) if r.DocHash in vectors else 0      # noqa: E731
        for first, k in ((0, 60), (5, 10), (59, 5), (0, 1)):
            pages = di.RerankByVector(qvec.tolist(), windows, first, k)
            for q, (rows, page) in enumerate(zip(windows, pages)):
                order = sorted(range(len(rows)), key=lambda j: (-value(rows[j], q), j))[first:first + k]
                assert [r.DocHash for r in page.Results] == [rows[j].DocHash for j in order], (q, first, k)
                assert [r.FinalRank for r in page.Results] == [rows[j].FinalRank for j in order]
                assert list(page.Scores) == [value(rows[j], q) for j in order]
        assert max(len(w) for w in windows) > 10
        # a window shorter than the page
        ghost = windows[0][:3]
        pages = di.RerankByVector(qvec[:1].tolist(), [ghost], 0, 3)
        assert sorted(r.DocHash for r in pages[0].Results) == sorted(r.DocHash for r in ghost)
    check_all()
    # the table is registered again on the scorer an ApplyDelta re-creates, with the ids as they stand then
    page = doc[17]
    before = {"docHash": page, "title": {t: row[page] for t, row in corpus["title"].items() if page in row},
              "body": {t: row[page] for t, row in corpus["body"].items() if page in row}, "children": corpus["children"][page],
              "anchors": {}}
    word = corpus["word"]
    after = {"docHash": page, "title": {h(word[3]): [1.0, 0.0]},
             "body": {h(word[3]): [0.25, 4.0, 9.0], h(word[40]): [1.0, 0.0, 1.0], h("brandnewword"): [0.5, 3.0]},
             "children": corpus["children"][page] + [h("http://site/never-seen-before")], "anchors": {}}
    di.ApplyDelta(forw, inv, before, after)
    check_all()
    di.SetDocVectors({})
    with pytest.raises(RuntimeError, match="SetDocVectors"):
        di.VectorSearch(qvec.tolist(), 5)
