"""DeviceIndex.BestPassages (the host mirror's snippet anchor, ss_best_passages underneath) on the config-1 corpus of
test_gpu_host.py: every row RetrieveBatch returned, against the numpy model (tests/passage_model.py) fed the same tokens and the
corpus' own position lists."""
import numpy as np
import pytest

from tests import passage_model as pm
from tests.test_gpu_host import corpus, host  # noqa: F401  (module fixtures of the host-mirror test)

pytestmark = pytest.mark.gpu


def test_host_mirror_best_passages(host, corpus):
    from tests.test_gpu_host import _weighted_tables, h
    forw, inv = _weighted_tables(host, corpus)
    di = host.DeviceIndex()
    di.load(forw, inv)
    word_id = {w: i for i, w in enumerate(sorted(corpus["body"]))}
    doc_id = {d: i for i, d in enumerate(sorted({d for docs in corpus["body"].values() for d in docs}))}
    lists = {(word_id[w], doc_id[d]): np.array(v[1:], np.float32) for w, docs in corpus["body"].items() for d, v in docs.items()}
    n_terms, n_docs = len(word_id), len(doc_id)

    def check(query, words, rows, width):
        got = di.BestPassages(query, rows, width) if width != 20 else di.BestPassages(query, rows)
        assert len(got) == len(rows)
        tokens = [word_id.get(h(w), n_terms) for w in words]
        seen = {"passage": 0, "multi": 0, "none": 0}
        for r, p in zip(rows, got):
            e = pm.best_window(*pm.occurrences(lists, n_terms, n_docs, tokens, doc_id.get(r.DocHash, n_docs)), tokens, width)
            assert p.HasPassage == bool(e["n_occ"]) and (p.Distinct, p.Occurrences) == (int(e["n_distinct"]), int(e["n_occ"]))
            assert (p.Start, p.Last) == (float(e["start"]), float(e["last"]))
            assert p.Words == list(dict.fromkeys(h(w) for i, w in enumerate(words) if int(e["token_mask"]) >> i & 1))
            assert len(p.Words) == p.Distinct
            seen["passage"] += p.HasPassage
            seen["multi"] += p.Distinct > 1
            seen["none"] += not p.HasPassage
        return seen
    query, words = "w3 w40 w149 notaword w3", ["w3", "w40", "w149", "notaword", "w3"]
    rows = di.RetrieveBatch([query], 30)[0]
    seen = check(query, words, rows, 20)
    assert len(rows) == 30 and seen["passage"] > 0
    wide = check(query, words, rows, 100000)
    assert wide["passage"] == seen["passage"] and wide["multi"] >= seen["multi"] and wide["multi"] > 0
    check(query, words, rows, 1)
    # title hits (anchor words of uncrawled children: no body posting, no passage), and a phrase whose words count as tokens
    assert check("w120", ["w120"], di.RetrieveBatch(["w120"], 50)[0], 20)["none"] > 0
    query = 'w7 "w1 w2"'
    check(query, ["w7", "w1", "w2"], di.RetrieveBatch([query], 20)[0], 5)
    # operators are read only when switched on: '-w40' is then no token, '+w3' a plain word
    query = "+w3 -w40"
    rows = di.RetrieveBatch([query], 20)[0]
    check(query, ["w3", "w40"], rows, 20)
    di.SetQueryOperators(True)
    rows = di.RetrieveBatch([query], 20)[0]
    check(query, ["w3"], rows, 20)
    di.SetQueryOperators(False)
    # no rows, no words
    rows = di.RetrieveBatch(["w3"], 2)[0]
    assert di.BestPassages("w3", []) == [] and [p.HasPassage for p in di.BestPassages("", rows)] == [False, False]
