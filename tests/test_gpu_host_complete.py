"""DeviceIndex.Complete and SetPrefixQueries (the host mirror of "results while you type", ss_lexicon_complete underneath) on the
config-1 corpus of test_gpu_host.py with an in-memory forw[0].  What a prefix query must return is computed by engine.Scorer.score_topk
on the very tables the DeviceIndex holds (read back from its snapshot), with the completions of the model as its terms."""
import json
import struct

import numpy as np
import pytest

from tests import lexicon_complete_model as cm
from tests.test_gpu_host import corpus, host  # noqa: F401  (module fixtures of the host-mirror test)

pytestmark = pytest.mark.gpu

MAX_QUERY_TERMS = 64
UNKNOWN = 0xFFFFFFFF


def read_snapshot(path):
    """-> (doc_names, term_names, {table: (term_ptr, post_doc, post_w, mag)}): the SSNAP002 layout of retrieval.hpp (FlatCorpus)"""
    blob = open(path, "rb").read()
    assert blob[:8] == b"SSNAP002"
    at = 8
    n, T, K = struct.unpack_from("<3Q", blob, at)
    at += 24

    def names(count):
        nonlocal at
        out = []
        for _ in range(count):
            (ln,) = struct.unpack_from("<I", blob, at)
            out.append(blob[at + 4:at + 4 + ln].decode())
            at += 4 + ln
        return out

    def array(dtype, count):
        nonlocal at
        a = np.frombuffer(blob, dtype=dtype, count=count, offset=at).copy()
        at += a.nbytes
        return a

    docs, terms, _ = names(n), names(T), names(K)
    tables = {}
    for name in ("title", "body"):
        P, n_pos = struct.unpack_from("<2Q", blob, at)
        at += 16
        term_ptr, post_doc, post_w = array(np.uint64, T + 1), array(np.uint32, P), array(np.float32, P)
        array(np.uint64, P + 1)
        array(np.float32, n_pos)
        tables[name] = (term_ptr, post_doc, post_w, array(np.float64, n))
    return docs, terms, tables


def test_host_mirror_completions_and_prefix_queries(host, corpus, ss_ctx, tmp_path):
    from spaghettisearch_amd import engine
    from tests.test_gpu_host import _weighted_tables, h
    forw, inv = _weighted_tables(host, corpus)
    d = corpus["doc"]
    planted = {"page": {d[5]: [0.5, 3.0], d[9]: [0.25, 1.0], d[12]: [0.5, 2.0]}, "pager": {d[5]: [0.5, 4.0], d[20]: [1.0, 0.0]},
               "pagerank": {d[7]: [1.0, 0.0], d[9]: [0.5, 5.0]}, "pagefault": {d[8]: [1.0, 2.0]}, "pagoda": {d[30]: [1.0, 1.0]}}
    for w, row in planted.items():
        inv[1].set(h(w), json.dumps(row))
    vocab = list(corpus["word"]) + list(planted)
    for w in vocab:
        forw[0].set(h(w), w)
    di = host.DeviceIndex()
    di.load(forw, inv)
    with pytest.raises(RuntimeError):
        di.Complete("pag")                                                     # no lexicon yet
    di.SetLexicon(forw[0])
    path = str(tmp_path / "corpus.ssnap")
    di.save_snapshot(path)
    docs, terms, tables = read_snapshot(path)
    tid = {t: i for i, t in enumerate(terms)}
    # ---- Complete against the model fed the same words (in term id order) and freq = title + body list length
    freq_of = {w: len(corpus["title"].get(h(w), {})) + len(corpus["body"].get(h(w), {})) for w in corpus["word"]}
    freq_of.update({w: len(planted[w]) for w in planted})
    word_of = {h(w): w for w in vocab}
    words = [word_of[t].encode() for t in terms]
    freq = np.array([freq_of[word_of[t]] for t in terms], dtype=np.uint32)

    def model(pre, m, min_freq=1):
        t, f, n, _ = cm.complete(words, freq, [pre.encode()], min_freq, m)
        return [(words[t[0, r]].decode(), int(f[0, r])) for r in range(n[0])]

    for pre, m, min_freq in (("pag", 10, 1), ("pag", 2, 1), ("w1", 10, 1), ("w1", 64, 1), ("", 5, 1), ("pager", 10, 2), ("zzz", 10, 1), ("w", 10, 10 ** 9)):
        got = di.Complete(pre, m, min_freq)
        assert all(isinstance(c.Word, str) for c in got)
        assert [(c.Word, c.Freq) for c in got] == model(pre, m, min_freq), (pre, m, min_freq)
    assert [c.Word for c in di.Complete("pag")] == ["page", "pager", "pagerank", "pagefault", "pagoda"]       # the defaults: m 10, min_freq 1
    # ---- prefix queries: the expected rows from engine.Scorer.score_topk on the same tables
    ti = engine.InvertedIndex(ss_ctx, len(docs), *tables["title"][:3])
    bi = engine.InvertedIndex(ss_ctx, len(docs), *tables["body"][:3])
    ti.set_weighted(tables["title"][3])
    bi.set_weighted(tables["body"][3])
    sc = engine.Scorer(ss_ctx, ti, bi)

    def expected(term_words, query_len, k=50):
        q_terms = np.array([tid.get(h(w), UNKNOWN) if w is not None else UNKNOWN for w in term_words], dtype=np.uint32)
        hits, n_hits = sc.score_topk(np.array([0, len(q_terms)], np.uint32), q_terms, k, query_len=np.array([query_len], np.int32))
        return [(docs[int(x["doc"])], float(x["final"]), float(x["title"]), float(x["body"])) for x in hits[0, :n_hits[0]]]

    def rows(res):
        return [(r.DocHash, r.FinalRank, r.TitleRank, r.BodyRank) for r in res]

    try:
        off = di.RetrieveBatch(["pag*", "pag* w3", "pag w3"], 50)
        assert rows(off[0]) == [] and rows(off[1]) == rows(off[2]) and len(off[2]) > 0                          # off: the star is a separator, as ever
        with pytest.raises(RuntimeError):
            di.SetPrefixQueries(33)
        with pytest.raises(RuntimeError):
            di.SetPrefixQueries(-1)
        di.SetPrefixQueries(4)
        four = ["page", "pager", "pagerank", "pagefault"]
        got = di.RetrieveBatch(["pag*", " ".join(four), "w3 PAG* w40", 'w3 "w2 pag*" w40', "w3 w40", "zzz* w3", "w3 *", "a*b w3"], 50)
        # the four most frequent completions as OR terms, the docs of the written-out query row for row, scored as ONE typed word
        assert [r.DocHash for r in got[0]] == [r.DocHash for r in got[1]] and len(got[0]) == 6
        assert rows(got[0]) == expected(four, 1)
        assert rows(got[1]) == expected(four, 4)
        assert rows(got[2]) == expected(["w3", "w40"] + four, 3)                                                  # behind the words, lower-cased
        assert rows(got[3]) == rows(di.RetrieveBatch(['w3 "w2 pag" w40'], 50)[0]) and len(got[3]) > 0       # a phrase is untouched
        assert rows(got[5]) == expected(["w3", None], 2)                                                          # no completion: one unknown word
        assert rows(got[6]) == expected(["w3"], 1) and rows(got[7]) == expected(["a", "b", "w3"], 3)             # no prefix tokens
        # the cut at SS_MAX_QUERY_TERMS: 61 words and two prefix tokens of up to 32 completions each
        di.SetPrefixQueries(32)
        w1 = [w for w, _ in model("w1", 32)]
        assert len(w1) == 32
        got = di.RetrieveBatch([" ".join(["w0"] * 61) + " pag* w1*", " ".join(["w0"] * 64) + " pag*"], 50)
        pag = [w for w, _ in model("pag", 32)]
        assert rows(got[0]) == expected(["w0"] * 61 + (pag + w1)[:3], 63)
        assert rows(got[1]) == expected(["w0"] * 64, 65)
        # with query operators "+word*" and "-word*" stay operator tokens; a plain prefix token is still read
        di.SetPrefixQueries(4)
        di.SetQueryOperators(True)
        got = di.RetrieveBatch(["w3 +w40*", "w3 -w40*", "w3 pag* -w40"], 50)
        di.SetPrefixQueries(0)
        want = di.RetrieveBatch(["w3 +w40", "w3 -w40"], 50)
        assert rows(got[0]) == rows(want[0]) and rows(got[1]) == rows(want[1])
        w40 = {r.DocHash for r in di.RetrieveBatch(["+w40"], 1000)[0]}
        di.SetQueryOperators(False)
        assert rows(got[2]) == [r for r in expected(["w3"] + four, 2, 1000) if r[0] not in w40][:50] and len(got[2]) > 0
        # ---- the refusals: entry points that refuse operators refuse the setting; no lexicon after load()
        di.SetPrefixQueries(4)
        di.SetDocGroups({})
        with pytest.raises(RuntimeError, match="prefix queries"):
            di.RetrieveBatchCollapsed(["w3"], 50, 1)
        di.load(forw, inv)                                                        # drops the lexicon; the setting stays
        assert not di.HasLexicon()
        assert len(di.RetrieveBatch(["w3 w40"], 50)[0]) > 0                      # no prefix token: nothing is asked of the lexicon
        with pytest.raises(RuntimeError, match="SetLexicon"):
            di.RetrieveBatch(["pag*"], 50)
        di.SetLexicon(forw[0])
        assert rows(di.RetrieveBatch(["pag*"], 50)[0]) == expected(four, 1)
    finally:
        sc.close()
        ti.close()
        bi.close()
