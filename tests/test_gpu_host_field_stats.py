"""GPU: the host mirror's field stats and histograms (DeviceIndex.FieldStats / FieldHistogram through pybind) on the golden 300 x 80 index,
loaded through the reference-shaped tables, against the model (tests/field_stats_model.py) that tests/test_gpu_field_stats.py holds the
engine calls to, with and without SetQueryOperators; 50 of the 300 docs have no field values and count as missing."""
import numpy as np
import pytest

from tests import field_stats_model as sm
from tests.test_gpu_host import h, host  # noqa: F401  (module fixture of the host-mirror test)
from tests.test_gpu_host_facet import DAY, NOW, NO_VALUE, golden_tables

pytestmark = pytest.mark.gpu


def test_field_stats_and_histograms_follow_the_model(host):
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
    with pytest.raises(RuntimeError, match="SetDocFields"):
        di.FieldStats(queries, [], [0])
    with pytest.raises(RuntimeError, match="SetDocFields"):
        di.FieldHistogram(queries, [], 0, 0, 1, 4)
    di.SetDocFields({doc[d]: (NOW - (d % 40) * DAY, 1000 + 37 * d) for d in range(250)})
    values = np.full((2, n_docs), NO_VALUE, dtype=np.int64)
    values[0, :250] = NOW - (np.arange(250) % 40) * DAY
    values[1, :250] = 1000 + 37 * np.arange(250)
    values = values[:, by_hash]
    clauses = [[(0, NOW - 20 * DAY, NOW)], [], [(1, 0, 100000)], [(0, NOW - 35 * DAY, NOW), (1, 2000, 9000)], [], [], [(0, NO_VALUE, NO_VALUE)]]
    with pytest.raises(RuntimeError, match="one list of ranges"):
        di.FieldStats(queries, [[]], [0])
    with pytest.raises(RuntimeError, match="phrases"):
        di.FieldHistogram(['w1 "w2 w3"'], [], 0, 0, 1, 4)
    with pytest.raises(RuntimeError):
        di.FieldStats(queries, [], [2])                                          # no such field: the library's refusal comes through
    weeks = [NOW - 40 * DAY + 7 * DAY * i for i in range(7)]                     # six bins of a week by edges; the values lie 0 .. 39 days back
    hists = [dict(field=0, origin=NOW - 39 * DAY, width=DAY, n_bins=40), dict(field=1, origin=2000, width=777, n_bins=9),
             dict(field=0, edges=weeks), dict(field=1, edges=[0, 1000, 1001, 5000, 2 ** 40])]
    seen = missing = 0
    for ops, terms in ((False, plain), (True, with_ops)):
        di.SetQueryOperators(ops)
        q_ptr, q_terms = pairs(terms)
        for cl in (None, clauses):
            ranges = None if cl is None else (pairs([[0] * len(cs) for cs in cl])[0], [c for cs in cl for c in cs])
            kw = dict(req=pairs(req) if ops else None, exc=pairs(exc) if ops else None, ranges=ranges)
            for fields in ([0], [1, 0], [1, 1, 0, 0]):
                stats, n_match, _ = sm.field_stats(n_docs, title, body, q_ptr, q_terms, values, fields, **kw)
                got = di.FieldStats(queries, [] if cl is None else cl, fields)
                assert len(got) == len(queries)
                for q, row in enumerate(got):
                    assert row.Total == int(n_match[q]) and len(row.Fields) == len(fields)
                    for i, f in enumerate(row.Fields):
                        assert (f.Min, f.Max, f.SumLo, f.SumHi, f.Count, f.Missing) == stats[q, i].tolist(), (ops, cl is None, fields, q, i)
                        if f.Count:
                            assert abs(f.Mean() - (f.SumHi * 2 ** 64 + f.SumLo) / f.Count) <= 1e-9 * abs(f.Mean())
                        seen += f.Count
                        missing += f.Missing
            for hk in hists:
                n_bins = hk.get("n_bins", len(hk.get("edges", [0])) - 1)
                counts, tails, _ = sm.field_histogram(n_docs, title, body, q_ptr, q_terms, values, hk["field"], n_bins, hk.get("origin", 0),
                                                      hk.get("width", 1), hk.get("edges"), **kw)
                if "edges" in hk:
                    got = di.FieldHistogram(queries, [] if cl is None else cl, hk["field"], edges=hk["edges"])
                else:
                    got = di.FieldHistogram(queries, [] if cl is None else cl, hk["field"], hk["origin"], hk["width"], n_bins)
                for q, row in enumerate(got):
                    assert list(row.Counts) == counts[q].tolist(), (ops, cl is None, hk, q)
                    assert (row.Below, row.Above, row.Missing, row.Total) == tails[q].tolist()
            assert [c.Total for c in di.FacetCounts(queries, [] if cl is None else cl)] == n_match.tolist()
    assert seen > 500 and missing > 50
    di.SetQueryOperators(False)
