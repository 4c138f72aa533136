"""GPU: the host mirror's near-duplicate filter (DeviceIndex.SetNearDuplicates / RetrieveBatchDeduped through pybind) on the config-1
corpus of test_gpu_host.py with one page made a copy of another apart from one word."""
import copy

import pytest

from tests.test_gpu_host import _weighted_tables, corpus, h, host  # noqa: F401  (module fixtures of the host-mirror test)

pytestmark = pytest.mark.gpu

N_SLOTS, MIN_MATCH = 32, 28


def test_a_copy_disappears_and_comes_back_after_a_delta(host, corpus):
    doc, word = corpus["doc"], corpus["word"]
    mine = copy.deepcopy({k: corpus[k] for k in ("children", "cats", "title", "body")})
    n_words = {}
    for row in mine["body"].values():
        for d in row:
            n_words[d] = n_words.get(d, 0) + 1
    a = max(doc[:1000], key=lambda d: (n_words.get(d, 0), d))                  # the crawled page with the most body words
    b = doc[12] if a != doc[12] else doc[13]
    a_words = [t for t, row in mine["body"].items() if a in row]
    assert len(a_words) >= 25
    # page b's body = page a's, one word short: its signature can differ from a's only in the slots where that word held the minimum
    # (one slot in len(a_words) on average), while unrelated pages of this corpus share well under half of their words
    query_words = [w for w in word if h(w) in a_words][:2]
    left_out = [t for t in a_words if t not in {h(w) for w in query_words}][-1]
    for t, row in mine["body"].items():
        row.pop(b, None)
        if a in row and t != left_out:
            row[b] = list(row[a])
    forw, inv = _weighted_tables(host, mine)
    di = host.DeviceIndex()
    di.load(forw, inv)
    queries = [" ".join(query_words), "notaword"]
    with pytest.raises(RuntimeError, match="SetNearDuplicates"):
        di.RetrieveBatchDeduped(queries, 1000, MIN_MATCH)
    with pytest.raises(RuntimeError):
        di.SetNearDuplicates(5)                                                # not one of 4, 8, .., 32
    assert di.NearDuplicateSlots() == 0
    di.SetNearDuplicates(N_SLOTS)
    assert di.NearDuplicateSlots() == N_SLOTS and not di.HasDocView()          # the view was only borrowed
    window = di.RetrieveBatch(queries, 1000)[0]
    names = [r.DocHash for r in window]
    assert a in names and b in names and len(window) < 1000
    first_of_pair = min(names.index(a), names.index(b))
    pages = di.RetrieveBatchDeduped(queries, 1000, MIN_MATCH, 0, 1000)
    got = [r.DocHash for r in pages[0].Results]
    assert got == [n for j, n in enumerate(names) if n not in (a, b) or j == first_of_pair]   # the later of the two is gone, nothing else
    assert list(pages[0].Similar) == [2 if n in (a, b) else 1 for n in got] and pages[0].Kept == len(window) - 1
    assert [(r.FinalRank, r.TitleRank, r.BodyRank, r.PageRank) for r in pages[0].Results] == \
           [(r.FinalRank, r.TitleRank, r.BodyRank, r.PageRank) for j, r in enumerate(window) if names[j] in got]
    assert len(pages[1].Results) == 0 and pages[1].Kept == 0
    paged = di.RetrieveBatchDeduped(queries, 1000, MIN_MATCH, 3, 5)[0]
    assert [r.DocHash for r in paged.Results] == got[3:8] and paged.Kept == len(window) - 1
    with pytest.raises(RuntimeError):
        di.RetrieveBatchDeduped(queries, 1000, N_SLOTS + 1)                    # more than the signatures' slots
    # page b is crawled again with another body: the signatures are built again behind the delta and both pages stay
    before = {"docHash": b, "title": {t: row[b] for t, row in mine["title"].items() if b in row},
              "body": {t: row[b] for t, row in mine["body"].items() if b in row}, "children": mine["children"][b], "anchors": {}}
    after = {"docHash": b, "title": before["title"],
             "body": {h(query_words[0]): [0.5, 1.0, 2.0], h(query_words[1]): [0.25, 7.0], h("brandnewword"): [0.25, 3.0]},
             "children": mine["children"][b], "anchors": {}}
    di.ApplyDelta(forw, inv, before, after)
    assert di.NearDuplicateSlots() == N_SLOTS
    window = di.RetrieveBatch(queries, 1000)[0]
    page = di.RetrieveBatchDeduped(queries, 1000, MIN_MATCH, 0, 1000)[0]
    names = [r.DocHash for r in window]
    assert a in names and b in names
    assert [r.DocHash for r in page.Results] == names and list(page.Similar) == [1] * len(names) and page.Kept == len(names)
    di.SetNearDuplicates(0)
    assert di.NearDuplicateSlots() == 0
    with pytest.raises(RuntimeError, match="SetNearDuplicates"):
        di.RetrieveBatchDeduped(queries, 1000, MIN_MATCH)
