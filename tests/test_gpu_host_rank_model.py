"""DeviceIndex.SetRankModel / RetrieveBatchRanked (the host mirror's learned ranking: ss_score_topk_masked -> ss_hit_proximity ->
ss_rerank_hits_by_model underneath) on the config-1 corpus of test_gpu_host.py: the page against the numpy model
(tests/rank_model_model.py) fed the window RetrieveBatch returns, the spans HitProximity returns for it and the tokeniser's
query length."""
import numpy as np
import pytest

from tests import rank_model_model as rm
from tests.test_gpu_host import corpus, host  # noqa: F401  (module fixtures of the host-mirror test)

pytestmark = pytest.mark.gpu

HIT = np.dtype([("doc", "<u4"), ("_pad", "<u4"), ("title", "<f8"), ("body", "<f8"), ("pagerank", "<f8"), ("final", "<f8")])


def test_host_mirror_ranked(host, corpus):
    from tests.test_gpu_host import _weighted_tables
    forw, inv = _weighted_tables(host, corpus)
    di = host.DeviceIndex()
    di.load(forw, inv)
    with pytest.raises(RuntimeError):
        di.RetrieveBatchRanked(["w3"], 30)                                            # no model yet
    # final + twice the closeness of the words, a tree on the window position and one on the words present; no fields, no vectors
    linear = np.zeros(rm.N_FEATURES)
    linear[[3, 8]] = [1.0, 2.0]
    trees = [rm.tree(rm.split(4, 4.0, 1, 2), rm.leaf(0.0), rm.leaf(0.125)), rm.tree(rm.split(6, 1.0, 1, 2, 1), rm.leaf(-0.25), rm.split(5, 3.0, 3, 4), rm.leaf(0.5), rm.leaf(1.0)),
             rm.tree(rm.split(11, 0.0, 1, 2, 1), rm.leaf(0.0625), rm.leaf(100.0))]     # the field column is absent: NaN goes left
    m = rm.model(rm.N_FEATURES, trees, linear, 0.5)
    ptr, nodes = rm.flat(m["trees"])
    with pytest.raises(RuntimeError):
        di.SetRankModel([], 0.0, [0, 3], [(0, 0, 2, 0, 0.5), (-1, 0, 0, 0, 1.0), (-1, 0, 0, 0, 2.0)])   # left == own index: refused by the library
    di.SetRankModel(linear.tolist(), 0.5, ptr.tolist(), nodes.tolist())
    for q_str, q_len, first, k in (("w3 w40 w149 notaword w3", 5, 0, 10), ("w3 w40 w149 notaword w3", 5, 25, 10), ('w7 "w1 w2"', 3, 0, 8), ("w5", 1, 2, 50)):
        window = di.RetrieveBatch([q_str], 30)[0]
        spans = di.HitProximity(q_str, window)
        n = len(window)
        hits, prox = np.zeros((1, n), dtype=HIT), np.zeros((1, n), dtype=rm.PROXIMITY)
        hits["doc"] = 0                                                                # (inside the table; the model reads no doc id without fields)
        for j, (r, p) in enumerate(zip(window, spans)):
            hits[0, j]["title"], hits[0, j]["body"], hits[0, j]["pagerank"], hits[0, j]["final"] = r.TitleRank, r.BodyRank, r.PageRank, r.FinalRank
            prox[0, j]["start"], prox[0, j]["end"], prox[0, j]["n_present"], prox[0, j]["n_occ"] = p.Start, p.End, p.Present, p.Occurrences
        o_hits, o_n, o_sc = rm.rerank(m, hits, [n], 1, first, k, prox=prox, query_len=[q_len])
        page = di.RetrieveBatchRanked([q_str], 30, first, k)[0]
        assert len(page.Results) == int(o_n[0]) > 0
        assert page.Scores == o_sc[0, : o_n[0]].tolist()
        assert [(r.FinalRank, r.TitleRank, r.BodyRank, r.PageRank) for r in page.Results] == \
            [(float(h["final"]), float(h["title"]), float(h["body"]), float(h["pagerank"])) for h in o_hits[0, : o_n[0]]]
    batch = ["w3", "notaword", "w40 w3"]
    assert [len(p.Results) for p in di.RetrieveBatchRanked(batch, 30, 0, 5)] == [min(5, len(w)) for w in di.RetrieveBatch(batch, 30)]
    di.SetQueryOperators(True)
    with pytest.raises(RuntimeError):
        di.RetrieveBatchRanked(["w3"], 30)
    di.SetQueryOperators(False)
