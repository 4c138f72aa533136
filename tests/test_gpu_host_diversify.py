"""GPU: the host mirror's diversified page (DeviceIndex.DiversifyByVector through pybind) on the config-1 corpus of test_gpu_host.py,
against the model (tests/diversify_model.py) by docHash.  The walk breaks ties by window position, never by the mirror's dense ids, so
the pages are compared exactly; the engine's call is compared byte for byte in test_gpu_diversify.py."""
import numpy as np
import pytest

from tests import diversify_model as dm
from tests.test_gpu_host import _weighted_tables, corpus, h, host  # noqa: F401  (module fixtures of the host-mirror test)

pytestmark = pytest.mark.gpu

DIM = 64
HIT_DTYPE = np.dtype([("doc", "<u4"), ("_pad", "<u4"), ("title", "<f8"), ("body", "<f8"), ("pagerank", "<f8"), ("final", "<f8")])


def test_diversify_follows_the_model(host, corpus):
    forw, inv = _weighted_tables(host, corpus)
    doc = corpus["doc"]
    di = host.DeviceIndex()
    di.load(forw, inv)
    rng = np.random.default_rng(43)
    queries = ["w3 w40 w149", "w120", 'w7 "w1 w2"', "w0"]
    windows = di.RetrieveBatch(queries, 60)
    assert max(len(w) for w in windows) > 10
    qvec = rng.integers(-8, 9, (4, DIM)).astype(np.int8)
    with pytest.raises(RuntimeError, match="SetDocVectors"):
        di.DiversifyByVector(qvec.tolist(), windows, 2, 1)
    with pytest.raises(RuntimeError, match="SetDocVectors"):
        di.DiversifyByVector([], windows, 2, 1)
    # a vector for the first 900 pages, none (the zero vector) for the rest; few distinct values: near-duplicates and ties
    named = 900
    vec = np.zeros((len(doc), DIM), np.int8)
    vec[:named, :6] = rng.integers(-8, 9, (named, 6))
    vec[7] = vec[3]
    di.SetDocVectors({doc[i]: vec[i].tolist() for i in range(named)})
    at = {d: i for i, d in enumerate(doc)}
    ghost = di.ScoreDocs("w0", [h("http://nowhere/")])[0]        # a row whose doc hash the index does not hold
    windows = [list(w) for w in windows]
    windows[0].insert(2, ghost)
    windows[3].append(ghost)
    k_in = max(len(w) for w in windows)
    hits = np.zeros((4, k_in), HIT_DTYPE)
    n_hits = np.array([len(w) for w in windows], np.int32)
    for q, w in enumerate(windows):
        for j, r in enumerate(w):
            hits["doc"][q, j] = at.get(r.DocHash, len(doc))        # the model's ids: positions in the corpus, the ghost outside
            hits["_pad"][q, j] = j
    with pytest.raises(RuntimeError, match="one window per query vector"):
        di.DiversifyByVector(qvec[:3].tolist(), windows, 2, 1)
    with pytest.raises(RuntimeError, match="ss_diversify_hits"):
        di.DiversifyByVector(qvec.tolist(), windows, 65537, 1)
    for by_rank in (False, True):
        for w_rel, w_div in ((2, 1), (30, 1), (1, 0), (0, 1)):
            for first, k in ((0, 60), (5, 10), (0, 1), (k_in - 2, 5), (k_in + 3, 2)):
                pages = di.DiversifyByVector([] if by_rank else qvec.tolist(), windows, w_rel, w_div, first, k)
                want = dm.diversify(None if by_rank else qvec, vec, hits, n_hits, w_rel, w_div, first, k, np.zeros((4, k), HIT_DTYPE),
                                    np.zeros(4, np.int32), np.zeros((4, k), dm.INFO_DTYPE))
                for q, page in enumerate(pages):
                    n = int(want[1][q])
                    rows = [windows[q][j] for j in want[0]["_pad"][q, :n]]
                    assert [r.DocHash for r in page.Results] == [r.DocHash for r in rows], (by_rank, w_rel, w_div, first, k, q)
                    assert [r.FinalRank for r in page.Results] == [r.FinalRank for r in rows]
                    assert list(page.Rel) == want[2]["rel"][q, :n].tolist() and list(page.Sim) == want[2]["sim"][q, :n].tolist()
    # the ghost row comes last, with no relevance and no similarity
    page = di.DiversifyByVector(qvec.tolist(), windows, 2, 1, 0, k_in)[0]
    assert page.Results[-1].DocHash == ghost.DocHash and (page.Rel[-1], page.Sim[-1]) == (dm.NO_SCORE, dm.NO_SCORE)
    assert page.Sim[0] == dm.NO_SCORE and len(page.Results) == len(windows[0])
    di.SetDocVectors({})
    with pytest.raises(RuntimeError, match="SetDocVectors"):
        di.DiversifyByVector([], windows, 2, 1)
