"""DeviceIndex.SetLexicon / WordList / SuggestWords (the host mirror of the reference's /wordlist/{pre} route and "did you mean",
ss_lexicon_* underneath) on the config-1 corpus of test_gpu_host.py with an in-memory forw[0]."""
import json

import pytest

from tests import lexicon_model as lm
from tests.test_gpu_host import corpus, host  # noqa: F401  (module fixtures of the host-mirror test)

pytestmark = pytest.mark.gpu


def test_host_mirror_word_list_and_suggestions(host, corpus):
    from tests.test_gpu_host import _weighted_tables, h
    forw, inv = _weighted_tables(host, corpus)
    d = corpus["doc"]
    planted = {"pagerank": {d[5]: [0.5, 3.0], d[9]: [0.25, 1.0, 8.0]}, "pagefault": {d[5]: [0.5, 4.0]}, "w3x": {d[7]: [1.0, 0.0]},
               "nohash": {d[8]: [1.0, 2.0]}}
    for w, row in planted.items():
        inv[1].set(h(w), json.dumps(row))
    vocab = list(corpus["word"]) + ["pagerank", "pagefault", "w3x"]            # "nohash" is a term, but forw[0] does not know it
    for w in vocab:
        forw[0].set(h(w), w)
    di = host.DeviceIndex()
    di.load(forw, inv)
    assert not di.HasLexicon()
    with pytest.raises(RuntimeError):
        di.WordList("w")
    di.SetLexicon(forw[0])
    assert di.HasLexicon()
    # the word list by prefix against sorted(): the term without a word is the one empty word, listed under the empty prefix only
    every = sorted([w.encode() for w in vocab] + [b""])
    for pre in ("", "w", "w1", "w14", "w149", "page", "pagerank", "pagerankx", "x"):
        want = [w for w in every if w.startswith(pre.encode())]
        assert di.WordList(pre, 0, 1000) == want
        assert di.WordList(pre, 3, 7) == want[3:10]
    assert di.WordList("w") == sorted(w.encode() for w in vocab if w.startswith("w"))[:50]        # the defaults: first 0, k 50
    # suggestions: only for the tokens the index does not know, each once
    got = di.SuggestWords("pagernak w3 W40 pagernak w3y zzzzzzzz")
    assert [s.Token for s in got] == ["pagernak", "w3y", "zzzzzzzz"]
    assert got[0].Words == ["pagerank"] and got[0].Distances == [1] and got[0].Freqs == [2]
    assert got[2].Words == [] and got[2].Distances == []
    # "w3y": against the model fed the same words and freq = title + body list length
    freq = {w: len(corpus["title"].get(h(w), {})) + len(corpus["body"].get(h(w), {})) for w in corpus["word"]}
    freq.update({w: len(planted[w]) for w in ("pagerank", "pagefault", "w3x")})
    words = sorted(vocab, key=h)                                                   # any order: the row is compared as (dist, -freq) keys
    terms, dist, n_out = lm.suggest([w.encode() for w in words], [freq[w] for w in words], [b"w3y"], 2, 1, 5)
    want_keys = [(int(dist[0, r]), -freq[words[terms[0, r]]]) for r in range(n_out[0])]
    assert len(got[1].Words) == n_out[0] == 5
    assert [(dd, -f) for dd, f in zip(got[1].Distances, got[1].Freqs)] == want_keys
    assert [lm.osa(b"w3y", w.encode()) for w in got[1].Words] == got[1].Distances and [freq[w] for w in got[1].Words] == got[1].Freqs
    wide = di.SuggestWords("pagernak", 3, 10)
    assert wide[0].Words[:1] == ["pagerank"] and "pagefault" not in wide[0].Words and di.SuggestWords("w3 w40") == []
    # a delta that brings a new word re-creates the lexicon; one that only moves postings updates the frequencies
    forw[0].set(h("pagerang"), "pagerang")
    page = d[11]
    before = {"docHash": page, "title": {}, "body": {}, "anchors": {}, "children": corpus["children"].get(page, [])}
    after = dict(before, body={h("pagerang"): [1.0, 0.0], h("pagefault"): [0.5, 1.0]})
    di.ApplyDelta(forw, inv, before, after)
    assert di.WordList("pager") == [b"pagerang", b"pagerank"]
    got = di.SuggestWords("pagernag pagefaul")
    assert got[0].Words[:1] == ["pagerang"] and got[1].Words == ["pagefault"] and got[1].Freqs == [2]
    di.ApplyDelta(forw, inv, after, dict(before, body={h("pagefault"): [0.5, 1.0]}))
    assert di.SuggestWords("pagernag")[0].Words == ["pagerank"]                    # "pagerang" has no posting left: freq 0 < 1
    assert di.WordList("pager") == [b"pagerang", b"pagerank"]                      # ... but it is still a word of the list
