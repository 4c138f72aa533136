"""GPU: the host mirror's vector lists (DeviceIndex.SetVectorLists / VectorSearchProbed through pybind) on the config-1 corpus of
test_gpu_host.py, against the model (tests/vector_lists_model.py) by docHash.  Dense ids are the mirror's own, so among rows of equal
score any candidate of that score is right; the engine's calls are compared byte for byte in test_gpu_vector_lists.py."""
import numpy as np
import pytest

from tests import vector_lists_model as vlm
from tests import vector_model as vm
from tests.test_gpu_host import _weighted_tables, corpus, h, host  # noqa: F401  (module fixtures of the host-mirror test)

pytestmark = pytest.mark.gpu

DIM, N_LISTS = 64, 5


def test_probed_search_follows_the_model_and_survives_a_new_scorer(host, corpus):
    forw, inv = _weighted_tables(host, corpus)
    doc = corpus["doc"]
    di = host.DeviceIndex()
    di.load(forw, inv)
    rng = np.random.default_rng(43)
    qvec = rng.integers(-128, 128, (4, DIM)).astype(np.int8)
    cent = rng.integers(-128, 128, (N_LISTS, DIM)).astype(np.int8)
    with pytest.raises(RuntimeError, match="SetDocVectors"):
        di.SetVectorLists(N_LISTS, cent.tolist())
    named = 900
    vec = np.zeros((len(doc), DIM), np.int8)                   # a vector for the first 900 pages, the zero vector for the rest
    vec[:named] = rng.integers(-128, 128, (named, DIM))
    di.SetDocVectors({doc[i]: vec[i].tolist() for i in range(named)})
    with pytest.raises(RuntimeError, match="SetVectorLists"):
        di.VectorSearchProbed(qvec.tolist(), 5, 2)
    with pytest.raises(RuntimeError, match="length"):
        di.SetVectorLists(1, [[1] * 65])
    with pytest.raises(RuntimeError, match="n_lists"):
        di.SetVectorLists(2, cent[:1].tolist())
    di.SetVectorLists(N_LISTS, cent.tolist())
    lists = vlm.assign(vec, cent)[0]                           # by score and list id only: the same under any dense ids
    score = vm.scores(qvec, vec)
    at = {d: i for i, d in enumerate(doc)}

    def check_all():
        for n_probe in (1, 2, N_LISTS, 99):
            pr = vlm.probes(qvec, cent, n_probe)
            for k in (1, 10, 50):
                rows = di.VectorSearchProbed(qvec.tolist(), k, n_probe)
                for q in range(4):
                    cand = np.flatnonzero(np.isin(lists, pr[q]))
                    want = sorted((int(score[q, i]) for i in cand), reverse=True)[:k]
                    got = [(r.DocHash, r.Score) for r in rows[q]]
                    assert [s for _, s in got] == want, (n_probe, k, q)
                    assert len({d for d, _ in got}) == len(want)
                    for d, s in got:
                        assert lists[at[d]] in pr[q] and int(score[q, at[d]]) == s
        # every list probed: VectorSearch's scores
        exact = di.VectorSearch(qvec.tolist(), 20)
        probed = di.VectorSearchProbed(qvec.tolist(), 20, N_LISTS)
        assert [[r.Score for r in row] for row in probed] == [[r.Score for r in row] for row in exact]
        # a mask: only pages 100 .. 399
        di.SetDocMasks({"some": [doc[i] for i in range(100, 400)]})
        rows = di.VectorSearchProbed(qvec.tolist(), 20, 2, ["some", "", "some", ""])
        pr = vlm.probes(qvec, cent, 2)
        for q in (0, 2):
            cand = [i for i in range(100, 400) if lists[i] in pr[q]]
            assert [r.Score for r in rows[q]] == sorted((int(score[q, i]) for i in cand), reverse=True)[:20]
    check_all()
    # the lists are assigned and registered again on the scorer an ApplyDelta re-creates, with the ids as they stand then
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
    # a later SetDocVectors clears them
    di.SetDocVectors({doc[i]: vec[i].tolist() for i in range(named)})
    with pytest.raises(RuntimeError, match="SetVectorLists"):
        di.VectorSearchProbed(qvec.tolist(), 5, 2)
    di.SetVectorLists(N_LISTS, cent.tolist())
    di.SetVectorLists(0, [])
    with pytest.raises(RuntimeError, match="SetVectorLists"):
        di.VectorSearchProbed(qvec.tolist(), 5, 2)
