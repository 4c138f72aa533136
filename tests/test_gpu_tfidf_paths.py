"""GPU side of the TF-IDF path suite: the kernels of csrc/tfidf.hip on the tables of tests/tfidf_cases.py, against the oracle.

tests/test_tfidf_cases_cpu.py shows on the CPU that every table reaches the path it is named after and that every float64 sum of a
case is exact in any order, so everything here is compared BIT FOR BIT (NaN against NaN: the sign and payload of a generated NaN
are not defined by the reference; +-inf and +-0 by their bits).  No tolerance, no skip: a case that cannot be compared fails.

Per case, under the case's options and again with "tfidf.bucket_min" = 1 << 62 (one float64 atomic per posting):
  ss_tfidf_build               idf of the live terms, weights, magnitudes  ==  oracle.tfidf
  ss_index_refresh_magnitudes  the same magnitudes                          (k_scatter<false>, k_bucket_sum<false>)
  ss_tfidf_build once more     weights == float32(w1 * idf), magnitudes == the oracle run on w1  (term_weighting.go:42 multiplies in place)
"""
import functools

import numpy as np
import pytest

from tests import tfidf_cases as tc

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = np.isnan(want)
    bad = np.nonzero((np.isnan(got) != nan) | (~nan & (bits(got) != bits(want))))[0]
    assert not len(bad), (what, f"{len(bad)} differ, first at {bad[:5].tolist()}: got {got[bad[:5]].tolist()} want {want[bad[:5]].tolist()}")


@functools.lru_cache(maxsize=2)
def reference(name):
    """the oracle's two builds of a case, computed once and shared by the bucketed and the atomic run"""
    from oracle import pyoracle
    return tc.expected(tc.get_case(name), pyoracle.tfidf)


@pytest.mark.parametrize("atomic", [False, True], ids=["partitioned", "atomic"])
@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_build_refresh_rebuild(ss_ctx, oracle, name, atomic):
    from spaghettisearch_amd import engine
    case = tc.get_case(name)
    idf_ref, (w1_ref, m1_ref), (w2_ref, m2_ref) = reference(name)
    opts = tc.lib_options(case.options)
    if atomic:
        opts["tfidf.bucket_min"] = 1 << 62
    tp = np.asarray(case.term_ptr, dtype=np.int64)
    lens = np.diff(tp)
    live = lens > 0
    ix = engine.InvertedIndex(ss_ctx, case.n_docs, case.term_ptr, case.post_doc, np.array(case.tf))
    try:
        if "df_extra" in case.options:
            ix.set_doc_freq((lens + np.asarray(case.options["df_extra"], dtype=np.int64)).astype(np.uint64))
        with ss_ctx.options(**{k.replace(".", "__"): v for k, v in opts.items()}):
            w1, m1, idf = ix.tfidf_build(case.total_docs)
            m1r = ix.refresh_magnitudes()
            w2, m2, idf2 = ix.tfidf_build(case.total_docs)
            m2r = ix.refresh_magnitudes()
    finally:
        ix.close()
    assert_same(idf[live], idf_ref[live], "idf")
    assert_same(w1, w1_ref, "weights")
    assert_same(m1, m1_ref, "magnitudes")
    assert_same(m1r, m1_ref, "magnitudes, refreshed")
    assert_same(idf2[live], idf_ref[live], "idf, second build")
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        assert_same(w2, (w1 * np.repeat(idf, lens)).astype(np.float32), "second build: float32(w1 * idf)")
    assert_same(w2, w2_ref, "second build: weights")
    assert_same(m2, m2_ref, "second build: magnitudes")
    assert_same(m2r, m2_ref, "second build: magnitudes, refreshed")
