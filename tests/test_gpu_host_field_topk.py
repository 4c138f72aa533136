"""GPU: the host mirror's field-ordered retrieval (DeviceIndex.RetrieveBatchByField through pybind) on the golden 300 x 80 index, loaded
through the reference-shaped tables, against the model (tests/field_topk_model.py), with and without SetQueryOperators; the rows are
those ScoreDocs gives for the same docs."""
import numpy as np
import pytest

from tests import field_topk_model as tm
from tests.test_gpu_host import h, host  # noqa: F401  (module fixture of the host-mirror test)
from tests.test_gpu_host_facet import DAY, NOW, NO_VALUE, golden_tables

pytestmark = pytest.mark.gpu


def test_retrieve_by_field_follows_the_model(host):
    z, n_docs, n_terms, doc, forw, inv = golden_tables(host)
    di = host.DeviceIndex()
    di.load(forw, inv)
    # the mirror numbers its docs in ascending hash order, and ties go by doc id: the model works in that numbering
    by_hash = np.argsort(np.array(doc))                                         # mirror order -> golden doc
    rank = np.empty(n_docs, dtype=np.int64)
    rank[by_hash] = np.arange(n_docs)

    def renumber(ptr, docs):
        out = rank[np.asarray(docs, dtype=np.int64)]
        for t in range(len(ptr) - 1):
            out[int(ptr[t]):int(ptr[t + 1])].sort()
        return ptr, out.astype(np.uint32)

    title, body = renumber(z["t_ptr"], z["t_doc"]), renumber(z["b_ptr"], z["b_doc"])
    doc_of = [doc[int(d)] for d in by_hash]                                     # mirror order -> hash
    queries = ["w3 w40 w79", "w12", "notaword", "w0 w1 w2 w3 w4", "w5 +w6 -w7", "", "w9 w9 notaword"]
    # operators off: '+' and '-' are punctuation, every word is a token; on: "+w6" is required (and stays a token), "-w7" excluded
    plain = [[3, 40, 79], [12], [], [0, 1, 2, 3, 4], [5, 6, 7], [], [9, 9]]
    with_ops = plain[:4] + [[5, 6]] + plain[5:]
    scored_as = {False: queries, True: queries[:4] + ["w5 w6"] + queries[5:]}  # the tokens ScoreDocs sees (it reads no operators)
    req = [[], [], [], [], [6], [], []]
    exc = [[], [], [], [], [7], [], []]
    pairs = lambda rows: (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32),                      # noqa: E731
                          np.array([t for r in rows for t in r], dtype=np.uint32))
    with pytest.raises(RuntimeError, match="SetDocFields"):
        di.RetrieveBatchByField(queries, [], 0)
    # a date and a size for 250 pages, none for the rest; the dates repeat every 40 docs, so ties are decided by the doc order
    di.SetDocFields({doc[d]: (NOW - (d % 40) * DAY, 1000 + 37 * d) for d in range(250)})
    values = np.full((2, n_docs), NO_VALUE, dtype=np.int64)
    values[0, :250] = NOW - (np.arange(250) % 40) * DAY
    values[1, :250] = 1000 + 37 * np.arange(250)
    values = values[:, by_hash]
    clauses = [[(0, NOW - 20 * DAY, NOW)], [], [(1, 0, 100000)], [(0, NOW - 35 * DAY, NOW), (1, 2000, 9000)], [], [], [(0, NO_VALUE, NO_VALUE)]]
    with pytest.raises(RuntimeError, match="one list of ranges"):
        di.RetrieveBatchByField(queries, [[]], 0)
    with pytest.raises(RuntimeError, match="phrases"):
        di.RetrieveBatchByField(['w1 "w2 w3"'], [], 0)
    seen = 0
    for ops, terms in ((False, plain), (True, with_ops)):
        di.SetQueryOperators(ops)
        q_ptr, q_terms = pairs(terms)
        for cl in (None, clauses):
            ranges = None if cl is None else (pairs([[0] * len(cs) for cs in cl])[0], [c for cs in cl for c in cs])
            for field, desc, first, k in ((0, True, 0, 10), (0, False, 3, 25), (1, True, 0, 300), (1, False, 40, 7)):
                want = tm.field_topk(n_docs, title, body, q_ptr, q_terms, values, field, desc, first, k, req=pairs(req) if ops else None,
                                     exc=pairs(exc) if ops else None, ranges=ranges)
                got = di.RetrieveBatchByField(queries, [] if cl is None else cl, field, desc, first, k)
                assert len(got) == len(queries)
                for q, page in enumerate(got):
                    assert [r.DocHash for r in page.Results] == [doc_of[int(d)] for d in want[0][q]], (ops, cl is None, field, desc, q)
                    assert list(page.Values) == want[1][q].tolist()
                    if page.Results:
                        rows = di.ScoreDocs(scored_as[ops][q], [r.DocHash for r in page.Results])
                        assert [(r.FinalRank, r.TitleRank, r.BodyRank) for r in page.Results] == [(r.FinalRank, r.TitleRank, r.BodyRank) for r in rows]
                    seen += len(page.Results)
            # the pages are cut from the docs FacetCounts counts
            assert [c.Total for c in di.FacetCounts(queries, [] if cl is None else cl)] == want[3].tolist()
    assert seen > 500
    di.SetQueryOperators(False)
