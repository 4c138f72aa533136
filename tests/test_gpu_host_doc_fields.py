"""GPU: the host mirror's doc fields (DeviceIndex.SetDocFields / RetrieveBatchFiltered / SortByField through pybind) on the config-1
corpus of test_gpu_host.py, against the model (tests/doc_fields_model.py) walked over the mirror's own RetrieveBatch rows, and the
Python wrappers end to end on the same definitions."""
import numpy as np
import pytest

from tests import doc_fields_model as fm
from tests.test_gpu_host import _weighted_tables, corpus, h, host  # noqa: F401  (module fixtures of the host-mirror test)

pytestmark = pytest.mark.gpu

DAY = 86400


def test_filtered_and_sorted_pages_follow_the_model_and_survive_a_delta(host, corpus):
    forw, inv = _weighted_tables(host, corpus)
    doc, word = corpus["doc"], corpus["word"]
    di = host.DeviceIndex()
    di.load(forw, inv)
    queries = ["w3 w40 w149", "w120", 'w7 "w1 w2"', "notaword", "w0"]
    with pytest.raises(RuntimeError, match="SetDocFields"):
        di.RetrieveBatchFiltered(queries, [[]] * 5)
    with pytest.raises(RuntimeError, match="SetDocFields"):
        di.SortByField(queries, 0, True, 100)
    # a date and a size for the first 900 pages (dates repeat: ties), none for the rest; a hash the index does not hold is ignored
    now = 1_700_000_000
    fields = {doc[i]: (now - (i % 40) * DAY, 1000 + 37 * i) for i in range(900)}
    di.SetDocFields({**fields, h("http://nowhere/"): (now, 1)})
    value = lambda r, f: fields[r.DocHash][f] if r.DocHash in fields else fm.NO_VALUE      # noqa: E731
    ranges = [[(0, now - 7 * DAY, now)], [(1, 0, 20000)], [(0, now - 20 * DAY, now), (1, 5000, 30000)], [(0, 0, now)], []]

    def check_all():
        narrowed = 0
        # the filtered rows are the first k rows of the whole ranking that match: walked over a window that holds the whole ranking
        whole = di.RetrieveBatch(queries, 1000)
        assert max(len(w) for w in whole) < 1000
        for k in (5, 50):
            rows = di.RetrieveBatchFiltered(queries, ranges, k)
            for q in range(len(queries)):
                want = [r for r in whole[q] if all(lo <= value(r, f) <= hi for f, lo, hi in ranges[q])][:k]
                assert [r.DocHash for r in rows[q]] == [r.DocHash for r in want], (q, k)
                assert [(r.FinalRank, r.TitleRank, r.BodyRank, r.PageRank) for r in rows[q]] == \
                       [(r.FinalRank, r.TitleRank, r.BodyRank, r.PageRank) for r in want]
                narrowed += 0 < len(want) and [r.DocHash for r in want] != [r.DocHash for r in whole[q][:k]]
        assert narrowed >= 3
        for field, desc, k_window, first, k in ((0, True, 100, 0, 10), (0, False, 100, 5, 10), (1, True, 1000, 0, 1000), (1, False, 30, 29, 4)):
            windows = di.RetrieveBatch(queries, k_window)
            pages = di.SortByField(queries, field, desc, k_window, first, k)
            for q, (rows, page) in enumerate(zip(windows, pages)):
                # (every row is a doc of the table: a page the map does not name holds NO_VALUE = INT64_MIN, first when ascending)
                order = sorted(range(len(rows)), key=lambda j: (-value(rows[j], field), j) if desc else (value(rows[j], field), j))
                want = [rows[j] for j in order][first:first + k]
                assert [r.DocHash for r in page.Results] == [r.DocHash for r in want], (q, field, desc)
                assert list(page.Values) == [value(r, field) for r in want]
    check_all()
    # the table is registered again on the scorer an ApplyDelta re-creates, with the ids as they stand then
    page = doc[17]
    before = {"docHash": page, "title": {t: row[page] for t, row in corpus["title"].items() if page in row},
              "body": {t: row[page] for t, row in corpus["body"].items() if page in row}, "children": corpus["children"][page],
              "anchors": {}}
    after = {"docHash": page, "title": {h(word[3]): [1.0, 0.0]},
             "body": {h(word[3]): [0.25, 4.0, 9.0], h(word[40]): [1.0, 0.0, 1.0], h("brandnewword"): [0.5, 3.0]},
             "children": corpus["children"][page] + [h("http://site/never-seen-before")], "anchors": {}}
    di.ApplyDelta(forw, inv, before, after)
    check_all()
    # with query operators the same call reads "+word" / "-word"
    di.SetQueryOperators(True)
    plus = di.RetrieveBatchFiltered(["w3 +w40", "w3 -w40"], [[(1, 0, 20000)], [(1, 0, 20000)]], 50)
    base = di.RetrieveBatch(["w3 +w40", "w3 -w40"], 1000)
    for q in range(2):
        assert [r.DocHash for r in plus[q]] == [r.DocHash for r in base[q] if 0 <= value(r, 1) <= 20000][:50]
    assert len(plus[0]) > 0 and len(plus[1]) > 0


def test_python_wrappers_end_to_end(ss_ctx):
    """Scorer.set_doc_fields / doc_field_masks / score_topk_filtered / sort_hits_by_field / hit_fields on a small synthetic index:
    the sets built on the device register as allow-lists and give the filtered call's rows"""
    from spaghettisearch_amd import engine, synth
    n_docs, n_terms = 5000, 200
    b = synth.zipf_index(n_docs, n_terms, 60000, seed=3)
    t = synth.zipf_index(n_docs, n_terms, 6000, seed=4)
    ti, bi = engine.InvertedIndex(ss_ctx, n_docs, *t), engine.InvertedIndex(ss_ctx, n_docs, *b)
    ti.tfidf_build(n_docs)
    bi.tfidf_build(n_docs)
    sc = engine.Scorer(ss_ctx, ti, bi)
    try:
        rng = np.random.default_rng(1)
        values = np.stack([rng.integers(0, 365, n_docs), rng.integers(100, 200000, n_docs)]).astype(np.int64)
        sc.set_doc_fields(values)
        buckets = [[(0, 0, 0)], [(0, 0, 6)], [(0, 0, 29)], [(0, 0, 364), (1, 100, 99999)]]      # past day / week / month, small pages
        words = sc.doc_field_masks(engine.pack_doc_ranges(buckets))
        assert words.tobytes() == fm.set_words(values, n_docs, buckets).tobytes()
        q_ptr, q_terms = synth.make_queries(12, 3, 100, seed=5)
        which = np.arange(12, dtype=np.int32) % 4
        hits, n_hits = sc.score_topk_filtered(q_ptr, q_terms, 30, ranges=engine.pack_doc_ranges([buckets[i] for i in which]))
        sc.set_doc_masks(words)
        ref, ref_n = sc.score_topk_masked(q_ptr, q_terms, which, 30)
        assert hits.tobytes() == ref.tobytes() and n_hits.tolist() == ref_n.tolist() and n_hits.max() > 0
        page, n_page, vals = sc.sort_hits_by_field(hits, n_hits, 0, 10, descending=True)
        want = fm.sort_page(hits, n_hits, values, n_docs, 0, True, 0, 10, np.zeros_like(page), np.zeros_like(n_page), np.zeros_like(vals))
        assert [page.tobytes(), n_page.tobytes(), vals.tobytes()] == [a.tobytes() for a in want]
        got = sc.hit_fields(page, n_page)
        assert got.tobytes() == fm.gather(page, n_page, values, n_docs, np.zeros_like(got)).tobytes()
    finally:
        sc.close()
        ti.close()
        bi.close()
