"""GPU parity: the doc-major view of an inverted table (ss_index_build_doc_view) and a doc's heaviest terms
(ss_index_doc_top_terms) vs the numpy model of tests/doc_view_model.py.  Selection and copying only: every comparison is bit-exact.
"""
import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine, synth
from tests import doc_view_model as dvm
from tests.test_gpu_score import tiny_index

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 6


def hand_table():
    """n_docs = 130, 200 terms.  Docs 0 and 129 are empty, doc 128 appears only in the last term, doc 5 in every term; row lengths
    0 (docs 0, 129, ...), 1 (doc 128), 63, 64, 65 (docs 10, 11, 12) and 200 (doc 5).  Weights: a different value per posting."""
    n_docs, T = 130, 200
    lists = [[5] for _ in range(T)]
    for d, n in ((10, 63), (11, 64), (12, 65)):
        for t in range(0, 2 * n, 2):                      # every other term: the rows interleave with doc 5's
            lists[t].append(d)
    lists[T - 1].append(128)
    lists[3] += [1, 127]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    doc = np.concatenate([np.sort(np.array(x, np.uint32)) for x in lists])
    w = (np.random.default_rng(5).permutation(len(doc)).astype(np.float32) + 1) / 8
    return n_docs, (ptr, doc, w)


def equal_row_table():
    """doc 1 holds 65 terms of ONE weight (the term order alone decides), doc 2 a row with both zeros, NaN, +-Inf and negatives."""
    special = np.array([np.nan, -2.0, np.inf, -np.inf, np.nan, -0.5, 7.0, 0.0, -0.0, 0.0, -0.0, 1e-45, -1e-45], np.float32)
    T = 65
    lists = [[1] for _ in range(T)]
    for t in range(len(special)):
        lists[5 * t].append(2)
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    doc = np.concatenate([np.array(x, np.uint32) for x in lists])
    w = np.full(len(doc), 2.5, np.float32)
    w[doc == 2] = special
    return 3, (ptr, doc, w)


TABLES = {
    "tiny": lambda: (5, tiny_index()[1]),
    "zipf": lambda: (3000, synth.zipf_index(3000, 500, 40000, seed=21)),
    "hand": hand_table,
    "equal-row": equal_row_table,
}


@pytest.fixture(scope="module", params=list(TABLES))
def table(request):
    """(n_docs, table, model view) — the model is computed once per table and shared"""
    n_docs, tab = TABLES[request.param]()
    return request.param, n_docs, tab, dvm.doc_view(*tab, n_docs)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_hand_table_has_the_rows_it_claims():
    n_docs, tab = hand_table()
    lens = np.diff(dvm.doc_view(*tab, n_docs)[0].astype(np.int64))
    assert lens[0] == lens[129] == 0 and lens[128] == 1 and lens[5] == 200 == len(tab[0]) - 1
    assert [int(lens[d]) for d in (10, 11, 12)] == [63, 64, 65]
    assert int(tab[1][-1]) == 128 and (tab[1][:-1] != 128).all()                    # doc 128: only in the last term


def test_view_equals_model_and_two_builds_give_identical_bytes(ss_ctx, table):
    _, n_docs, tab, view = table
    idx = engine.InvertedIndex(ss_ctx, n_docs, *tab)
    try:
        idx.build_doc_view()
        got = idx.read_doc_view()
        for g, want in zip(got, view):
            assert same_bits(g, want)
        idx.build_doc_view()                                                    # replaces the view
        again = idx.read_doc_view()
        assert all(same_bits(a, b) for a, b in zip(got, again))
    finally:
        idx.close()


def test_view_after_tfidf_build_holds_the_tfidf_weights(ss_ctx, oracle):
    n_docs = 3000
    tab = synth.zipf_index(n_docs, 500, 40000, seed=22)
    idx = engine.InvertedIndex(ss_ctx, n_docs, *tab)
    try:
        idx.build_doc_view()
        assert same_bits(idx.read_doc_view()[2], dvm.doc_view(*tab, n_docs)[2])  # tf before the build
        w, _, _ = idx.tfidf_build(n_docs)
        w_ref, _, _ = oracle.tfidf(*tab, n_docs, n_docs)
        assert same_bits(w, np.asarray(w_ref, np.float32))
        idx.build_doc_view()
        got = idx.read_doc_view()
        want = dvm.doc_view(tab[0], tab[1], w, n_docs)
        assert all(same_bits(a, b) for a, b in zip(got, want)) and not same_bits(got[2], dvm.doc_view(*tab, n_docs)[2])
    finally:
        idx.close()


def test_state_errors(ss_ctx):
    """No view before a build and after each call that changes postings or weights; ss_index_set_weighted leaves it."""
    n_docs = 3000
    tab = synth.zipf_index(n_docs, 500, 40000, seed=23)
    idx = engine.InvertedIndex(ss_ctx, n_docs, *tab)

    def no_view():
        for call in (idx.read_doc_view, idx.drop_doc_view, lambda: idx.doc_top_terms(np.array([1], np.uint32), 3)):
            with pytest.raises(SpaghettiError) as ei:
                call()
            assert ei.value.code == ERR_STATE
    try:
        no_view()
        idx.build_doc_view()
        idx.set_weighted(np.ones(n_docs))
        view = idx.read_doc_view()                                               # still there
        assert all(same_bits(a, b) for a, b in zip(view, dvm.doc_view(*tab, n_docs)))
        idx.tfidf_build(n_docs)
        no_view()
        idx.build_doc_view()
        tp, pd, pw = idx.read()
        idx.apply_delta(del_docs=np.array([7], np.uint32), add=(np.array([3], np.uint32), np.array([7], np.uint32), np.array([0.5], np.float32)))
        no_view()
        idx.build_doc_view()
        tp, pd, pw = idx.read()
        assert all(same_bits(a, b) for a, b in zip(idx.read_doc_view(), dvm.doc_view(tp, pd, pw, n_docs)))   # the view of the updated table
        idx.resize(n_docs + 10, 500)
        no_view()
        idx.build_doc_view()
        assert len(idx.read_doc_view()[0]) == n_docs + 11
        idx.drop_doc_view()
        no_view()
    finally:
        idx.close()


def docs_for(name, n_docs, view):
    lens = np.diff(view[0].astype(np.int64))
    rng = np.random.default_rng(3)
    docs = list(rng.integers(0, n_docs, size=40)) if n_docs > 200 else list(range(n_docs))
    docs += [n_docs - 1, int(np.argmax(lens)), int(np.argmin(lens)), n_docs - 1, int(np.argmax(lens))]     # the last doc, duplicates
    return np.array(docs, dtype=np.uint32)


@pytest.mark.parametrize("m", [1, 5, 64])
def test_doc_top_terms_equals_model(ss_ctx, table, m):
    """m below and above the row lengths (rows of 0 .. 200 entries), duplicate docs, the last doc; host outputs keep what lies past
    n_out[i]."""
    name, n_docs, tab, view = table
    idx = engine.InvertedIndex(ss_ctx, n_docs, *tab)
    try:
        idx.build_doc_view()
        docs = docs_for(name, n_docs, view)
        ref_t, ref_w, ref_n = dvm.top_terms(view, docs, m)
        terms, w, n = idx.doc_top_terms(docs, m)
        assert n.tolist() == ref_n.tolist()
        assert same_bits(terms, ref_t) and same_bits(w, ref_w)                  # zeros past n_out on both sides
        if m == 64:
            assert (ref_n < m).any()                                            # m above a row's length
        # sentinels past n_out stay, and the weights may be left out
        out = (np.full((len(docs), m), 0xABCDEF01, np.uint32), None, np.full(len(docs), -7, np.int32))
        t2, w2, n2 = idx.doc_top_terms(docs, m, out=out)
        assert w2 is None and n2.tolist() == ref_n.tolist()
        for i in range(len(docs)):
            assert t2[i, :ref_n[i]].tolist() == ref_t[i, :ref_n[i]].tolist() and (t2[i, ref_n[i]:] == 0xABCDEF01).all()
    finally:
        idx.close()


def test_doc_top_terms_device_outputs(ss_ctx, table):
    import torch
    name, n_docs, tab, view = table
    idx = engine.InvertedIndex(ss_ctx, n_docs, *tab)
    try:
        idx.build_doc_view()
        docs = docs_for(name, n_docs, view)
        m = 5
        ref_t, ref_w, ref_n = dvm.top_terms(view, docs, m)
        d_docs = torch.from_numpy(docs.view(np.int32)).cuda()
        out = (torch.full((len(docs), m), -3, dtype=torch.int32, device="cuda"), torch.full((len(docs), m), -3.0, dtype=torch.float32, device="cuda"),
               torch.full((len(docs),), -3, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        idx.doc_top_terms(d_docs, m, out=out)
        terms, w, n = (x.cpu().numpy() for x in out)
        assert n.tolist() == ref_n.tolist()
        for i in range(len(docs)):
            k = int(ref_n[i])
            assert terms[i, :k].view(np.uint32).tolist() == ref_t[i, :k].tolist() and w[i, :k].tobytes() == ref_w[i, :k].tobytes()
            assert (terms[i, k:] == -3).all() and (w[i, k:] == -3.0).all()      # untouched
    finally:
        idx.close()


def test_special_weights_by_hand(ss_ctx):
    """The row of doc 2 in equal_row_table: +Inf, 7, 1e-45, the four zeros by term, -1e-45, -0.5, -2, -Inf, the NaNs by term; doc 1:
    65 equal weights, terms 0 .. 64 in order."""
    n_docs, tab = equal_row_table()
    idx = engine.InvertedIndex(ss_ctx, n_docs, *tab)
    try:
        idx.build_doc_view()
        terms, w, n = idx.doc_top_terms(np.array([2, 1], np.uint32), 64)
        assert n.tolist() == [13, 64]
        assert (terms[0, :13] // 5).tolist() == [2, 6, 11, 7, 8, 9, 10, 12, 5, 1, 3, 0, 4]
        assert np.signbit(w[0, 3:7]).tolist() == [False, True, False, True]     # the stored zeros, not canonical ones
        assert np.isnan(w[0, 11:13]).all() and w[0, 0] == np.inf and w[0, 10] == -np.inf
        assert terms[1].tolist() == list(range(64)) and (w[1] == 2.5).all()
    finally:
        idx.close()


def test_rejected_arguments_leave_the_outputs_untouched(ss_ctx):
    n_docs, tab = hand_table()
    idx = engine.InvertedIndex(ss_ctx, n_docs, *tab)
    try:
        idx.build_doc_view()
        for docs, m in (([5], 0), ([5], 65), ([5, n_docs], 5), ([0xFFFFFFFF], 5)):
            mm = max(m, 1)
            out = (np.full((len(docs), mm), 77, np.uint32), np.full((len(docs), mm), 7.5, np.float32), np.full(len(docs), -1, np.int32))
            d = np.array(docs, np.uint32)
            with pytest.raises(SpaghettiError) as ei:                           # (straight to the library: the wrapper would size arrays by m)
                engine.check(idx.ctx.lib.ss_index_doc_top_terms(idx.h, len(d), d.ctypes.data, m, out[0].ctypes.data, out[1].ctypes.data,
                                                                out[2].ctypes.data), idx.ctx.h)
            assert ei.value.code == ERR_INVALID
            assert (out[0] == 77).all() and (out[1] == 7.5).all() and (out[2] == -1).all()
        terms, _, n = idx.doc_top_terms(np.array([n_docs - 1, 128], np.uint32), 64)    # the largest valid id still works
        assert n.tolist() == [0, 1] and terms[1, 0] == 199
    finally:
        idx.close()
