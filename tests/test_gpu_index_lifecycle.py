"""Refusals of the index object's entry points (csrc/index.hip) that no other test pins: each with its exact return code, and the table
(or the context) still usable afterwards.  The table of tests/test_gpu_tfidf.py::test_rejects_unsorted_and_out_of_range: 5 docs, 2 terms,
5 postings.  (A document frequency below the local list, ss_index_set_doc_freq(NULL) and phrase scoring without positions are reached
by tests/test_gpu_shard_index.py and tests/test_gpu_phrase.py; the former also sets document frequencies on a weighted table, but
asks for any error: here the code is pinned and the table read back.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SS_ERR_INVALID, SS_ERR_STATE = 1, 6
TP = np.array([0, 3, 5], dtype=np.uint64)
DOCS = np.array([0, 2, 4, 1, 3], dtype=np.uint32)
TF = np.array([.5, 1, .25, 1, .5], dtype=np.float32)
POS_PTR = np.array([0, 1, 2, 3, 4, 6], dtype=np.uint64)
POS = np.array([1, 2, 3, 4, 5, -100], dtype=np.float32)


def make(ss_ctx):
    from spaghettisearch_amd import engine
    return engine.InvertedIndex(ss_ctx, 5, TP, DOCS, TF)


def refused(code, fn, *args):
    from spaghettisearch_amd import SpaghettiError
    with pytest.raises(SpaghettiError) as e:
        fn(*args)
    assert e.value.code == code, (e.value.code, str(e.value))


def table_is_intact(idx):
    tp, pd, _ = idx.read()
    assert np.array_equal(tp, TP) and np.array_equal(pd, DOCS)


def test_set_positions_refusals_release_the_positions(ss_ctx):
    idx = make(ss_ctx)
    try:
        refused(SS_ERR_STATE, idx.read_positions)                              # none loaded yet
        for bad_ptr, pos in (([1, 1, 2, 3, 4, 6], POS),                        # pos_ptr[0] != 0
                             ([0, 2, 1, 3, 4, 6], POS),                        # decreasing
                             (POS_PTR, None)):                                 # NULL pos with a non-zero total
            idx.set_positions(POS_PTR, POS)
            pp, pv = idx.read_positions()
            assert np.array_equal(pp, POS_PTR) and np.array_equal(pv, POS)
            refused(SS_ERR_INVALID, idx.set_positions, np.array(bad_ptr, dtype=np.uint64), pos)
            refused(SS_ERR_STATE, idx.read_positions)                          # the refused call released what the table held
            table_is_intact(idx)
        refused(SS_ERR_INVALID, idx.set_positions, None, POS)                  # (no pos_ptr at all: nothing is touched)
        idx.set_positions(POS_PTR, POS)                                        # and the next valid call is taken
        pp, pv = idx.read_positions()
        assert np.array_equal(pp, POS_PTR) and np.array_equal(pv, POS)
        idx.set_positions(np.zeros(6, dtype=np.uint64), None)                  # a NULL pos with a zero total is fine
        assert idx.read_positions()[1].size == 0
    finally:
        idx.close()


def test_set_doc_freq_after_the_build_is_a_state_error(ss_ctx):
    idx = make(ss_ctx)
    try:
        df = np.array([4, 2], dtype=np.uint64)
        idx.set_doc_freq(df)
        w, mag, _ = idx.tfidf_build(8)
        refused(SS_ERR_STATE, idx.set_doc_freq, df)
        refused(SS_ERR_STATE, idx.set_doc_freq, None)
        table_is_intact(idx)
        assert np.array_equal(idx.read()[2], w) and np.array_equal(idx.refresh_magnitudes(), mag)
    finally:
        idx.close()


def test_destroy_while_a_scorer_holds_the_table(ss_ctx):
    from spaghettisearch_amd import engine
    ti, bi = make(ss_ctx), make(ss_ctx)
    sc = None
    try:
        ti.set_weighted(np.ones(5))
        bi.set_weighted(np.ones(5))
        sc = engine.Scorer(ss_ctx, ti, bi)
        for idx in (ti, bi):
            refused(SS_ERR_STATE, idx.close)
            assert idx.h                                                       # (the handle is still the table's)
            table_is_intact(idx)
        hits, n_hits = sc.score_topk(np.array([0, 1], dtype=np.uint32), np.array([0], dtype=np.uint32), 3)
        assert n_hits.tolist() == [3]
    finally:
        if sc is not None:
            sc.close()
        ti.close()
        bi.close()
    assert not ti.h and not bi.h


def test_create_refuses_a_term_ptr_that_does_not_start_at_zero(ss_ctx):
    from spaghettisearch_amd import engine
    refused(SS_ERR_INVALID, engine.InvertedIndex, ss_ctx, 5, np.array([1, 3, 5], dtype=np.uint64), DOCS, TF)
    idx = make(ss_ctx)                                                         # the context takes the next table
    try:
        table_is_intact(idx)
    finally:
        idx.close()
