"""DeviceIndex.HitProximity and RetrieveBatchProximity (the host mirror's term proximity, ss_hit_proximity and ss_score_topk_proximity /
ss_rerank_hits_by_proximity underneath) on the config-1 corpus of test_gpu_host.py: every row RetrieveBatch returned, against the
numpy model (tests/proximity_model.py) fed the same tokens and the corpus' own position lists."""
import numpy as np
import pytest

from tests import proximity_model as xm
from tests.test_gpu_host import corpus, host  # noqa: F401  (module fixtures of the host-mirror test)

pytestmark = pytest.mark.gpu


def test_host_mirror_proximity(host, corpus):
    from tests.test_gpu_host import _weighted_tables, h
    forw, inv = _weighted_tables(host, corpus)
    di = host.DeviceIndex()
    di.load(forw, inv)
    word_id = {w: i for i, w in enumerate(sorted(corpus["body"]))}
    doc_id = {d: i for i, d in enumerate(sorted({d for docs in corpus["body"].values() for d in docs}))}
    lists = {(word_id[w], doc_id[d]): np.array(v[1:], np.float32) for w, docs in corpus["body"].items() for d, v in docs.items()}
    n_terms, n_docs = len(word_id), len(doc_id)
    vocabulary = set(corpus["title"]) | set(corpus["body"])                     # a word of the titles alone has an id and no body posting

    def entry_of(words, doc_hash):
        tokens = [word_id.get(h(w), n_terms) for w in words]
        return xm.span_entry(xm.occurrences(lists, n_terms, n_docs, tokens, doc_id.get(doc_hash, n_docs)), tokens), tokens

    def same_span(p, e, words):
        assert p.HasSpan == bool(e["n_present"]) and (p.Present, p.Occurrences) == (int(e["n_present"]), int(e["n_occ"]))
        assert (p.Start, p.End) == (float(e["start"]), float(e["end"]))
        assert p.Words == list(dict.fromkeys(h(w) for i, w in enumerate(words) if int(e["token_mask"]) >> i & 1))
        assert len(p.Words) == p.Present

    query, words = "w3 w40 w149 notaword w3", ["w3", "w40", "w149", "notaword", "w3"]
    rows = di.RetrieveBatch([query], 30)[0]
    got = di.HitProximity(query, rows)
    assert len(got) == len(rows) == 30
    for r, p in zip(rows, got):
        same_span(p, entry_of(words, r.DocHash)[0], words)
    assert sum(p.Present > 1 for p in got) > 0 and sum(p.HasSpan for p in got) > 0
    assert di.HitProximity("w3", []) == [] and [p.HasSpan for p in di.HitProximity("", rows[:2])] == [False, False]
    # the page: the model's order of the same window, its scores and its spans; a second page; a quoted phrase takes the chained path
    for q_str, q_words, first, k in ((query, words, 0, 10), (query, words, 25, 10), ('w7 "w1 w2"', ["w7", "w1", "w2"], 0, 8)):
        window = di.RetrieveBatch([q_str], 30)[0]
        ent = [entry_of(q_words, r.DocHash) for r in window]
        big_t = len({h(w) if h(w) in vocabulary else None for w in q_words})     # an id per known word, one for all unknown ones
        score = [np.float64(0.5) * np.float64(r.FinalRank) + np.float64(2.0) * xm.bonus_of(e, big_t) for r, (e, _) in zip(window, ent)]
        order = sorted(range(len(window)), key=lambda j: (-float(score[j]), j))[first:first + k]
        page = di.RetrieveBatchProximity([q_str], 30, 0.5, 2.0, first, k)[0]
        assert [r.DocHash for r in page.Results] == [window[j].DocHash for j in order] and len(order) > 0
        assert [r.FinalRank for r in page.Results] == [window[j].FinalRank for j in order]
        assert page.Scores == [float(score[j]) for j in order]
        for p, j in zip(page.Spans, order):
            same_span(p, ent[j][0], q_words)
    di.SetQueryOperators(True)
    with pytest.raises(RuntimeError):
        di.RetrieveBatchProximity([query], 30)
    di.SetQueryOperators(False)
