"""GPU parity of the quoted-phrase kernels (k_phrase_match, k_phrase_close, their host plan) on the constructed cases of
tests/phrase_cases.py: part seams, close-ups whose source and destination overlap, the title-only pass, field mixing,
position-list edges, phrase lengths and the order of the float32 weight sum.

The truth is tests/phrase_model.py (the second restatement of retrieval/phrase.go), merged into the ranking by the C oracle
(`extra`); tests/test_phrase_cases_cpu.py ties that model to orc_phrase and proves that every case hits its condition.  Every
comparison is bit-exact.

k is capped at 1024, so a plain top-k sees a fraction of 16384 matches.  Doc masks make all of them observable: allow-lists
that tile the doc range in windows of WINDOW docs, the phrase query once per window with k = 1024, and the rows of every
window held against the oracle on the tables restricted to that window (the construction of
tests/test_gpu_doc_masks.py::test_phrase_queries).
"""
import time

import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, _lib, engine
from tests import phrase_cases as pc
from tests.test_gpu_doc_masks import restrict_table

pytestmark = pytest.mark.gpu

WINDOW = 1000           # docs per allow-list: below k = 1024 (no row is cut) and no divisor of the 8192-candidate parts


class Opened:
    """The two tables of a case with weights, magnitudes and positions loaded, and a scorer on them."""

    def __init__(self, ctx, case):
        self.ti = engine.InvertedIndex(ctx, case.n_docs, *case.title)
        self.bi = engine.InvertedIndex(ctx, case.n_docs, *case.body)
        self.ti.set_weighted(case.mag_t)
        self.bi.set_weighted(case.mag_b)
        self.ti.set_positions(*case.tpos)
        self.bi.set_positions(*case.bpos)
        self.sc = engine.Scorer(ctx, self.ti, self.bi)

    def __enter__(self):
        return self.sc

    def __exit__(self, *exc):
        self.sc.close()
        self.ti.close()
        self.bi.close()
        return False


def batch_of(queries):
    q_ptr, q_terms = pc.pack([q.terms for q in queries])
    p_ptr, p_terms = pc.pack([q.phrase for q in queries])
    return q_ptr, q_terms, p_ptr, p_terms


def restrict_extra(extra, lo, hi):
    if extra is None:
        return None
    keep = (extra[0] >= lo) & (extra[0] < hi)
    return tuple(a[keep] for a in extra)


def expected(oracle, case, q, k, tables=None, window=None):
    title, body = tables if tables is not None else (case.title, case.body)
    extra = case.extra(q)
    if window is not None:
        extra = restrict_extra(extra, *window)
    ref, _ = oracle.score_topk(case.n_docs, title, body, case.mag_t, case.mag_b, np.array(q.terms, np.uint32), k,
                               query_len=len(q.terms) + len(q.phrase), extra=extra)
    return ref


def assert_row(hits, n_hits, row, ref, what):
    n = int(n_hits[row])
    assert n == len(ref), (what, n, len(ref))
    assert hits["doc"][row, :n].tolist() == ref["doc"].tolist(), what
    for f in ("title", "body", "final"):
        assert np.array_equal(hits[f][row, :n].view(np.uint64), ref[f].view(np.uint64)), (what, f)
    assert not np.frombuffer(hits[row, n:].tobytes(), dtype=np.uint8).any(), (what, "rows past n_hits")


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_every_match_window_by_window(ss_ctx, oracle, name):
    case = pc.get_case(name)
    t0 = time.perf_counter()
    for q in case.queries:
        case.extra(q)
    t_model = time.perf_counter() - t0
    windows = [(lo, min(lo + WINDOW, case.n_docs)) for lo in range(0, case.n_docs, WINDOW)]
    allowed = np.zeros((len(windows), case.n_docs), dtype=bool)
    for i, (lo, hi) in enumerate(windows):
        allowed[i, lo:hi] = True
    assert allowed.sum(axis=0).tolist() == [1] * case.n_docs                    # the windows tile the doc range
    rows = [(q, w) for q in case.queries for w in range(len(windows))]
    q_ptr, q_terms, p_ptr, p_terms = batch_of([q for q, _ in rows])
    mask_id = np.array([w for _, w in rows], dtype=np.int32)
    with Opened(ss_ctx, case) as sc:
        sc.set_doc_masks(engine.pack_doc_masks(allowed, case.n_docs))
        t0 = time.perf_counter()
        hits, n_hits = sc.score_topk_masked(q_ptr, q_terms, mask_id, 1024, p_ptr=p_ptr, p_terms=p_terms)
        t_gpu = time.perf_counter() - t0
    tabs = [(restrict_table(case.title, a), restrict_table(case.body, a)) for a in allowed]
    union = {q.name: [] for q in case.queries}
    for row, (q, w) in enumerate(rows):
        ref = expected(oracle, case, q, 1024, tables=tabs[w], window=windows[w])
        assert len(ref) <= WINDOW
        assert_row(hits, n_hits, row, ref, (q.name, windows[w]))
        got = hits["doc"][row, :int(n_hits[row])]
        assert ((got >= windows[w][0]) & (got < windows[w][1])).all(), (q.name, w)
        union[q.name].append(got)
    n_match = 0
    for q in case.queries:
        if len(q.phrase) and not len(q.terms):          # a phrase alone: the rows of all windows ARE the match set, all of it
            docs = np.sort(np.concatenate(union[q.name]))
            assert docs.tolist() == case.model_phrase(q.phrase)[0].tolist(), q.name
            n_match += len(docs)
    print(f"\n{name}: {len(case.queries)} queries x {len(windows)} windows, {n_match} phrase-only matches seen; "
          f"model {t_model:.2f} s, masked call {t_gpu:.3f} s")


@pytest.mark.parametrize("small", [0, 1], ids=["small-kernel-off", "small-kernel-on"])
@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_unmasked_topk(ss_ctx, oracle, name, small):
    case = pc.get_case(name)
    q_ptr, q_terms, p_ptr, p_terms = batch_of(case.queries)
    ss_ctx.set_option("score.small", small)
    try:
        with Opened(ss_ctx, case) as sc:
            for k in (1, 64, 1024):
                hits, n_hits = sc.score_topk_phrase(q_ptr, q_terms, p_ptr, p_terms, k)
                for row, q in enumerate(case.queries):
                    assert_row(hits, n_hits, row, expected(oracle, case, q, k), (q.name, k))
    finally:
        ss_ctx.set_option("score.small", None)


def test_mixed_batch_sync_and_three_in_flight(ss_ctx, oracle):
    """Family G: phrases with 0, 1, 2 and 3 workgroup parts, plain OR queries, one phrase twice and phrases with an unknown word in
    one batch (per-query part counts and result-list offsets differ); the synchronous call, and three tickets in flight."""
    case = pc.get_case("G.batch")
    qs = case.queries
    q_ptr, q_terms, p_ptr, p_terms = batch_of(qs)
    names = [q.name for q in qs]
    a, b = names.index("G.C.both_fields"), names.index("G.C.both_fields.again")
    with Opened(ss_ctx, case) as sc:
        sync = {k: sc.score_topk_phrase(q_ptr, q_terms, p_ptr, p_terms, k) for k in (64, 1024)}
        for k, (hits, n_hits) in sync.items():
            for row, q in enumerate(qs):
                assert_row(hits, n_hits, row, expected(oracle, case, q, k), (q.name, k))
            assert int(n_hits[a]) > 0 and hits[a].tobytes() == hits[b].tobytes() and n_hits[a] == n_hits[b]
            for row, q in enumerate(qs):
                if q.claim.get("unknown") and not q.terms:
                    assert int(n_hits[row]) == 0
        for _ in range(2):
            t1 = sc.submit(q_ptr, q_terms, 1024, p_ptr=p_ptr, p_terms=p_terms)
            t2 = sc.submit(q_ptr, q_terms, 64, p_ptr=p_ptr, p_terms=p_terms)
            t3 = sc.submit(q_ptr, q_terms, 1024, p_ptr=p_ptr, p_terms=p_terms)
            for t, k in ((t2, 64), (t3, 1024), (t1, 1024)):
                hc, nc = sc.collect(t)
                assert hc.tobytes() == sync[k][0].tobytes() and nc.tolist() == sync[k][1].tolist(), k


def test_seventeen_terms_are_refused_and_nothing_is_written(ss_ctx, oracle):
    case = pc.get_case("F.lengths")
    (bad,) = case.errors
    good = next(q for q in case.queries if q.name.endswith("len16"))
    assert len(bad.phrase) == pc.PH_MAX + 1 and bad.claim["code"] == 7
    k = 8
    with Opened(ss_ctx, case) as sc:
        for batch in ([bad], [good, bad], [bad, good]):
            q_ptr, q_terms, p_ptr, p_terms = batch_of(batch)
            hits = np.frombuffer(bytes([0xA5]) * (len(batch) * k * engine.HIT_DTYPE.itemsize), dtype=engine.HIT_DTYPE).copy().reshape(len(batch), k)
            n_hits = np.full(len(batch), -77, dtype=np.int32)
            before = hits.tobytes()
            with pytest.raises(SpaghettiError) as e:
                _lib.check(ss_ctx.lib.ss_score_topk_phrase(sc.h, len(batch), q_ptr.ctypes.data, q_terms.ctypes.data, p_ptr.ctypes.data,
                                                           p_terms.ctypes.data, None, None, k, hits.ctypes.data, n_hits.ctypes.data), ss_ctx.h)
            assert e.value.code == 7                                             # SS_ERR_UNSUPPORTED
            assert hits.tobytes() == before and n_hits.tolist() == [-77] * len(batch)
            with pytest.raises(SpaghettiError) as e:
                sc.submit(q_ptr, q_terms, k, p_ptr=p_ptr, p_terms=p_terms)
            assert e.value.code == 7
            # the next valid call on the same scorer
            q_ptr, q_terms, p_ptr, p_terms = batch_of(case.queries)
            h2, n2 = sc.score_topk_phrase(q_ptr, q_terms, p_ptr, p_terms, k)
            for row, q in enumerate(case.queries):
                assert_row(h2, n2, row, expected(oracle, case, q, k), q.name)


def test_postings_added_without_positions_do_not_match_a_phrase(ss_ctx, oracle):
    """ss_index_apply_delta (not _pos) gives the new postings EMPTY position lists: listPos[1:] of a one-element row.  Such a posting
    is in no phrase, not even a one-term one, and is an ordinary posting for an OR term."""
    from tests.phrase_model import PhraseModel
    n_docs, n_terms = 12, 3
    tb = pc.Tables()
    for field in (pc.TITLE, pc.BODY):
        tb.add(field, 0, [1, 4, 7], pc.wt([1, 4, 7], field), [[3], [5, 9], [2]])
        tb.add(field, 1, [1, 2, 4, 5, 7, 9], pc.wt([1, 2, 4, 5, 7, 9], 5 + field), [[4], [4], [1], [6], [3], [1]])
    (title, tpos, _), (body, bpos, _) = tb.finish(n_docs, n_terms)
    ti = engine.InvertedIndex(ss_ctx, n_docs, *title)
    bi = engine.InvertedIndex(ss_ctx, n_docs, *body)
    sc = None
    try:
        ti.set_positions(*tpos)
        bi.set_positions(*bpos)
        add_t = np.array([0, 0, 2, 2], dtype=np.uint32)                    # word 0 arrives in docs 2 and 5, the new word 2 in docs 2 and 3
        add_d = np.array([2, 5, 2, 3], dtype=np.uint32)
        add_w = np.array([0.5, 0.25, 0.75, 0.125], dtype=np.float32)
        for idx in (ti, bi):
            _lib.check(ss_ctx.lib.ss_index_apply_delta(idx.h, 0, None, 0, None, None, len(add_t), add_t.ctypes.data, add_d.ctypes.data,
                                                       add_w.ctypes.data), ss_ctx.h)
            idx.n_post += len(add_t)
        tabs, poss, mags = [], [], []
        for idx in (ti, bi):
            tabs.append(idx.read())
            poss.append(idx.read_positions())
            ptr, doc, w = tabs[-1]
            mag = np.sqrt(np.bincount(doc.astype(np.int64), weights=(w * w).astype(np.float32).astype(np.float64), minlength=n_docs))
            mag[mag == 0] = 1.0
            mags.append(mag)
            idx.set_weighted(mag)
            pp = poss[-1][0].astype(np.int64)
            for t, d in zip(add_t.tolist(), add_d.tolist()):                # the new postings are there, with empty position lists
                j = int(ptr[t]) + doc[int(ptr[t]):int(ptr[t + 1])].tolist().index(d)
                assert pp[j + 1] == pp[j], (t, d)
        model = PhraseModel(tabs[0], tabs[1], poss[0], poss[1])
        assert model.phrase([0])[0].tolist() == [1, 4, 7]                    # not 2 and 5
        assert model.phrase([2])[0].tolist() == []                           # a word with empty lists only
        assert model.phrase([0, 1])[0].tolist() == [1, 7]                    # 4 - 1 = 3, 3 - 1 = 2; doc 2 and 5 hold both words
        sc = engine.Scorer(ss_ctx, ti, bi)
        queries = [pc.Query("p0", [], [0], {}), pc.Query("p2", [], [2], {}), pc.Query("p01", [], [0, 1], {}), pc.Query("p02", [], [0, 2], {}),
                   pc.Query("or0", [0], [], {}), pc.Query("or2", [2], [], {}), pc.Query("or2.p0", [2], [0], {}), pc.Query("p10", [], [1, 0], {})]
        q_ptr, q_terms, p_ptr, p_terms = batch_of(queries)
        hits, n_hits = sc.score_topk_phrase(q_ptr, q_terms, p_ptr, p_terms, 16)
        for row, q in enumerate(queries):
            extra = model.phrase(list(q.phrase)) if q.phrase else None
            ref, _ = oracle.score_topk(n_docs, tabs[0], tabs[1], mags[0], mags[1], np.array(q.terms, np.uint32), 16,
                                       query_len=len(q.terms) + len(q.phrase), extra=extra)
            assert_row(hits, n_hits, row, ref, q.name)
        by = {q.name: row for row, q in enumerate(queries)}
        assert sorted(hits["doc"][by["p0"], :int(n_hits[by["p0"]])].tolist()) == [1, 4, 7]
        assert int(n_hits[by["p2"]]) == 0
        assert sorted(hits["doc"][by["or0"], :int(n_hits[by["or0"]])].tolist()) == [1, 2, 4, 5, 7]      # the same word as a plain term
        assert sorted(hits["doc"][by["or2"], :int(n_hits[by["or2"]])].tolist()) == [2, 3]
    finally:
        if sc is not None:
            sc.close()
        ti.close()
        bi.close()
