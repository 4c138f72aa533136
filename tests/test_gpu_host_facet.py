"""GPU: the host mirror's facet counts (DeviceIndex.FacetCounts through pybind) on the golden 300 x 80 index, loaded through the
reference-shaped tables, against the set model (tests/facet_model.py), with and without SetQueryOperators."""
import json
import os

import numpy as np
import pytest

from tests import facet_model as fm
from tests.test_gpu_host import h, host  # noqa: F401  (module fixture of the host-mirror test)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_300x80.npz")
DAY = 86400
NOW = 1_700_000_000
NO_VALUE = -(2 ** 63)


def golden_tables(host):
    """the golden CSR tables as inv[0] / inv[1] rows {doc hash: [weight]} and forw[4] magnitudes; term t is the word "w<t>" """
    z = np.load(GOLDEN)
    n_docs, n_terms = int(z["n_docs"]), len(z["b_ptr"]) - 1
    doc = [h(f"http://golden/{d}") for d in range(n_docs)]
    forw = [host.MemDB() for _ in range(6)]
    inv = [host.MemDB() for _ in range(3)]
    for table, ptr, docs, w in ((inv[0], z["t_ptr"], z["t_doc"], z["t_w"]), (inv[1], z["b_ptr"], z["b_doc"], z["b_w"])):
        for t in range(n_terms):
            row = {doc[int(docs[j])]: [float(w[j])] for j in range(int(ptr[t]), int(ptr[t + 1]))}
            if row:
                table.set(h(f"w{t}"), json.dumps(row))
    for d in range(n_docs):
        forw[4].set(doc[d], json.dumps({"title": float(z["t_mag"][d]), "body": float(z["b_mag"][d])}))
    return z, n_docs, n_terms, doc, forw, inv


def test_facet_counts_follow_the_model(host):
    z, n_docs, n_terms, doc, forw, inv = golden_tables(host)
    di = host.DeviceIndex()
    di.load(forw, inv)
    title, body = (z["t_ptr"], z["t_doc"]), (z["b_ptr"], z["b_doc"])
    queries = ["w3 w40 w79", "w12", "notaword", "w0 w1 w2 w3 w4", "w5 +w6 -w7", "", "w9 w9 notaword"]
    # operators off: '+' and '-' are punctuation, every word is a token; on: "+w6" is required (and stays a token), "-w7" excluded
    plain = [[3, 40, 79], [12], [], [0, 1, 2, 3, 4], [5, 6, 7], [], [9, 9]]
    with_ops = plain[:4] + [[5, 6]] + plain[5:]
    req = [[], [], [], [], [6], [], []]
    exc = [[], [], [], [], [7], [], []]
    pairs = lambda rows: (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32),                      # noqa: E731
                          np.array([t for r in rows for t in r], dtype=np.uint32))

    def want(terms, ops, clauses, buckets, masks, values):
        q_ptr, q_terms = pairs(terms)
        ranges = None if clauses is None else (pairs([[0] * len(cs) for cs in clauses])[0], [c for cs in clauses for c in cs])
        return fm.facet_counts(n_docs, title, body, q_ptr, q_terms, masks=masks, fields=values, req=pairs(req) if ops else None,
                               exc=pairs(exc) if ops else None, ranges=ranges, buckets=buckets)

    def same(got, ref, names, n_b):
        assert [g.Total for g in got] == ref[0].tolist()
        assert [[g.Masks[n] for n in names] for g in got] == ref[1].tolist()
        assert [list(g.Buckets) for g in got] == ref[2].reshape(len(got), n_b).tolist()

    # totals alone: no masks, no fields
    for ops, terms in ((False, plain), (True, with_ops)):
        di.SetQueryOperators(ops)
        ref = want(terms, ops, None, [], None, None)
        same(di.FacetCounts(queries), ref, [], 0)
        assert ref[0].max() > 50 and ref[0][2] == 0
    di.SetQueryOperators(False)
    with pytest.raises(RuntimeError, match="SetDocFields"):
        di.FacetCounts(queries, [], [(0, 0, NOW)])
    with pytest.raises(RuntimeError, match="one list of ranges"):
        di.FacetCounts(queries, [[]])
    with pytest.raises(RuntimeError, match="phrases"):
        di.FacetCounts(['w1 "w2 w3"'])
    # masks by name (a hash the index does not hold is ignored), a date and a size for 250 pages, none for the rest
    names = ["even", "front"]                                                   # the mirror registers the sets in name order
    di.SetDocMasks({"front": [doc[d] for d in range(120)] + [h("http://nowhere/")], "even": [doc[d] for d in range(0, n_docs, 2)]})
    masks = np.zeros((2, n_docs), dtype=bool)
    masks[0, 0::2] = True
    masks[1, :120] = True
    di.SetDocFields({doc[d]: (NOW - (d % 40) * DAY, 1000 + 37 * d) for d in range(250)})
    values = np.full((2, n_docs), NO_VALUE, dtype=np.int64)
    values[0, :250] = NOW - (np.arange(250) % 40) * DAY
    values[1, :250] = 1000 + 37 * np.arange(250)
    buckets = [(0, NOW - DAY, NOW), (0, NOW - 7 * DAY, NOW), (0, NOW - 30 * DAY, NOW), (0, 0, NOW), (1, 0, 4999), (1, 5000, 2 ** 62),
               (0, NO_VALUE, NO_VALUE), (1, 10, 5)]
    clauses = [[(0, NOW - 20 * DAY, NOW)], [], [(1, 0, 100000)], [(0, NOW - 35 * DAY, NOW), (1, 2000, 9000)], [], [], [(0, NO_VALUE, NO_VALUE)]]
    for ops, terms in ((False, plain), (True, with_ops)):
        di.SetQueryOperators(ops)
        for cl in (None, clauses):
            ref = want(terms, ops, cl, buckets, masks, values)
            same(di.FacetCounts(queries, [] if cl is None else cl, buckets), ref, names, len(buckets))
            assert ref[1].sum() > 0 and ref[2][:, :6].sum(axis=0).min() > 0 and ref[2][:, 7].sum() == 0
        # the counts are those of the docs RetrieveBatchFiltered ranks
        rows = di.RetrieveBatchFiltered(queries, clauses, 1000)
        assert [len(r) for r in rows] == ref[0].tolist()
    assert want(with_ops, True, clauses, buckets, masks, values)[0].tolist() != want(plain, False, clauses, buckets, masks, values)[0].tolist()
    di.SetQueryOperators(False)
