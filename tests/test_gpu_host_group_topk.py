"""GPU: the host mirror's sites facet (DeviceIndex.TopGroups through pybind) on the golden 300 x 80 index, loaded through the
reference-shaped tables, against the model (tests/group_topk_model.py), with and without SetQueryOperators; the site keys come back as
the strings SetDocGroups was given."""
import numpy as np
import pytest

from tests import group_topk_model as gm
from tests.test_gpu_host import h, host  # noqa: F401  (module fixture of the host-mirror test)
from tests.test_gpu_host_facet import DAY, NOW, NO_VALUE, golden_tables

pytestmark = pytest.mark.gpu


def test_top_groups_follow_the_model(host):
    z, n_docs, n_terms, doc, forw, inv = golden_tables(host)
    di = host.DeviceIndex()
    di.load(forw, inv)
    by_hash = np.argsort(np.array(doc))                                         # mirror order -> golden doc
    rank = np.empty(n_docs, dtype=np.int64)
    rank[by_hash] = np.arange(n_docs)

    def renumber(ptr, docs):
        out = rank[np.asarray(docs, dtype=np.int64)]
        for t in range(len(ptr) - 1):
            out[int(ptr[t]):int(ptr[t + 1])].sort()
        return ptr, out.astype(np.uint32)

    title, body = renumber(z["t_ptr"], z["t_doc"]), renumber(z["b_ptr"], z["b_doc"])
    queries = ["w3 w40 w79", "w12", "notaword", "w0 w1 w2 w3 w4", "w5 +w6 -w7", "", "w9 w9 notaword"]
    plain = [[3, 40, 79], [12], [], [0, 1, 2, 3, 4], [5, 6, 7], [], [9, 9]]
    with_ops = plain[:4] + [[5, 6]] + plain[5:]
    req = [[], [], [], [], [6], [], []]
    exc = [[], [], [], [], [7], [], []]
    pairs = lambda rows: (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32),                      # noqa: E731
                          np.array([t for r in rows for t in r], dtype=np.uint32))
    with pytest.raises(RuntimeError, match="SetDocGroups"):
        di.TopGroups(queries)
    # 260 pages on 23 sites of unequal size, the rest on none; the mirror numbers a key by its rank among the distinct keys
    site = lambda d: "site%02d.example" % (d * d % 23)                                                                      # noqa: E731
    di.SetDocGroups({doc[d]: site(d) for d in range(260)})
    names = sorted({site(d) for d in range(260)})
    group = np.full(n_docs, gm.NO_GROUP, dtype=np.uint32)
    group[:260] = [names.index(site(d)) for d in range(260)]
    group = group[by_hash]
    di.SetDocFields({doc[d]: (NOW - (d % 40) * DAY, 1000 + 37 * d) for d in range(250)})
    values = np.full((2, n_docs), NO_VALUE, dtype=np.int64)
    values[0, :250] = NOW - (np.arange(250) % 40) * DAY
    values[1, :250] = 1000 + 37 * np.arange(250)
    values = values[:, by_hash]
    clauses = [[(0, NOW - 20 * DAY, NOW)], [], [(1, 0, 100000)], [(0, NOW - 35 * DAY, NOW), (1, 2000, 9000)], [], [], [(0, NO_VALUE, NO_VALUE)]]
    with pytest.raises(RuntimeError, match="one list of ranges"):
        di.TopGroups(queries, [[]])
    with pytest.raises(RuntimeError, match="phrases"):
        di.TopGroups(['w1 "w2 w3"'])
    seen = 0
    for ops, terms in ((False, plain), (True, with_ops)):
        di.SetQueryOperators(ops)
        q_ptr, q_terms = pairs(terms)
        for cl in (None, clauses):
            ranges = None if cl is None else (pairs([[0] * len(cs) for cs in cl])[0], [c for cs in cl for c in cs])
            for first, m in ((0, 10), (0, 1), (2, 5), (0, 40), (30, 3)):
                rows, n_out, n_groups, n_ungrouped, n_match, _ = gm.top_groups(n_docs, title, body, q_ptr, q_terms, group, first, m, fields=values,
                                                                               req=pairs(req) if ops else None, exc=pairs(exc) if ops else None,
                                                                               ranges=ranges)
                got = di.TopGroups(queries, [] if cl is None else cl, first, m)
                assert len(got) == len(queries)
                for q, page in enumerate(got):
                    assert [(k, c) for k, c in page.Rows] == [(names[int(g)], int(c)) for g, c in rows[q].tolist()], (ops, cl is None, first, m, q)
                    assert (page.Total, page.Groups, page.Ungrouped) == (int(n_match[q]), int(n_groups[q]), int(n_ungrouped[q]))
                    seen += len(page.Rows)
            assert [c.Total for c in di.FacetCounts(queries, [] if cl is None else cl)] == n_match.tolist()
    assert seen > 60
    di.SetQueryOperators(False)
