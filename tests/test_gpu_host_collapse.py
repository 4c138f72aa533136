"""GPU: the host mirror's collapsed result pages (DeviceIndex.SetDocGroups / RetrieveBatchCollapsed through pybind) on the config-1
corpus of test_gpu_host.py, against the sequential model (tests/collapse_model.py) walked over the mirror's own RetrieveBatch rows."""
import numpy as np
import pytest

from tests import collapse_model as cm
from tests.test_gpu_host import _weighted_tables, corpus, h, host  # noqa: F401  (module fixtures of the host-mirror test)

pytestmark = pytest.mark.gpu


def model_pages(rows, key_of, g, first, k):
    """rows: RetrieveBatch's rows of one query (the window) -> (DocHashes of the page, same, n_kept)"""
    names = sorted({r.DocHash for r in rows})
    ids = {n: i for i, n in enumerate(names)}
    keys = sorted({key_of[n] for n in names if n in key_of})
    group = np.array([keys.index(key_of[n]) if n in key_of else cm.NO_GROUP for n in names], np.uint32)
    kept, same = cm.collapse_row([ids[r.DocHash] for r in rows], group, g)
    page = kept[first:first + k]
    return [rows[j] for j in page], [same[j] for j in page], len(kept)


def test_collapsed_pages_follow_the_model_and_survive_a_delta(host, corpus):
    forw, inv = _weighted_tables(host, corpus)
    doc, word = corpus["doc"], corpus["word"]
    di = host.DeviceIndex()
    di.load(forw, inv)
    queries = ["w3 w40 w149", "w120", 'w7 "w1 w2"', "notaword", "w0"]
    with pytest.raises(RuntimeError, match="SetDocGroups"):
        di.RetrieveBatchCollapsed(queries, 100, 2)
    # seven sites over the first 700 pages (equal strings, one site), the rest unnamed; a hash the index does not hold is ignored
    key_of = {doc[i]: f"site-{i % 7}.example" for i in range(700)}
    di.SetDocGroups({**key_of, h("http://nowhere/"): "site-0.example"})

    def check_all():
        collapsed_something = 0
        for k_window, g, first, k in ((100, 2, 0, 50), (100, 2, 10, 10), (1000, 1, 0, 5), (1000, 3, 5, 1000), (30, 1, 29, 4)):
            windows = di.RetrieveBatch(queries, k_window)
            pages = di.RetrieveBatchCollapsed(queries, k_window, g, first, k)
            assert len(pages) == len(queries)
            for q, (rows, page) in enumerate(zip(windows, pages)):
                want_rows, want_same, want_kept = model_pages(rows, key_of, g, first, k)
                assert [r.DocHash for r in page.Results] == [r.DocHash for r in want_rows], (q, k_window, g, first, k)
                assert [(r.FinalRank, r.TitleRank, r.BodyRank, r.PageRank) for r in page.Results] == \
                       [(r.FinalRank, r.TitleRank, r.BodyRank, r.PageRank) for r in want_rows]
                assert list(page.Same) == want_same and page.Kept == want_kept
                collapsed_something += want_kept < len(rows)
            assert len(windows[3]) == 0 and pages[3].Kept == 0 and len(windows[0]) == min(k_window, len(windows[0]))
        assert collapsed_something > 0
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
    # an empty map is a table too: nothing is ever collapsed
    di.SetDocGroups({})
    rows = di.RetrieveBatch(queries[:1], 40)[0]
    page0 = di.RetrieveBatchCollapsed(queries[:1], 40, 1, 0, 40)[0]
    assert [r.DocHash for r in page0.Results] == [r.DocHash for r in rows] and list(page0.Same) == [1] * len(rows) and page0.Kept == len(rows)
