"""CPU side of the TF-IDF path suite (tests/tfidf_cases.py): everything a reviewer can check without a GPU.

  * Every case reaches the paths it is named after: its expect_paths are a subset of what the path model reports for its table and
    options, and every path the suite claims (tfidf_cases.REQUIRED_PATHS, REQUIRED_VALUE_PATHS) is reached by at least one case.
  * The exactness condition: for every case, both builds and every doc the float64 sum of the oracle's float32 squares is the exact
    rational sum in ANY order (integer multiples of one power of two that sum to less than 2^53; cross-checked against
    fractions.Fraction on the small tables).  That is what lets tests/test_gpu_tfidf_paths.py demand bit equality of the magnitudes.
    Docs with an inf or NaN square have no rational sum: the cases that hold some are listed (NONFINITE_CASES), each such doc holds
    one posting.
  * oracle.tfidf (C) and oracle_np.tfidf (numpy), two restatements of term_weighting.go, agree bit for bit on every case when the
    numpy one is given the C oracle's idf.
  * The model's constants are the ones in csrc/tfidf_plan.hpp.
"""
import numpy as np
import pytest

from tests import tfidf_cases as tc
from tests import tfidf_plan

_REACHED = {}          # case name -> paths reached (model + oracle values); read by test_every_path_has_a_case


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits_or_nan(got, want):
    """NaN against NaN (sign and payload of a generated NaN are not defined by the reference), everything else bit for bit"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def test_constants_match_the_source(tmp_path):
    """The model's constants are the ones the compiled header holds (tests/tfidf_plan_harness.cpp prints them); the host arithmetic the
    model restates is held against the header's, line by line, in tests/test_tfidf_plan_cpu.py."""
    got, _, _ = tfidf_plan.run(tfidf_plan.build(tmp_path))
    got["SC_PF"] *= got["SC_TPB"]                                            # (entries per thread -> the largest window the prefetch takes)
    want = {n: getattr(tc, n) for n in got}
    print(got)
    assert got == want
    assert set(got) == {"CH", "SC_CH", "SC_TPB", "SC_PT", "SC_WIN", "SC_PF", "SC_BPT_MAX", "NB_MAX", "HEAD_CAP", "HEAD_LEVELS", "HEAD_PIECE"}
    assert (tc.CH, tc.SC_CH, tc.SC_TPB, tc.NB_MAX, tc.HEAD_CAP, tc.HEAD_LEVELS, tc.HEAD_PIECE) == (4096, 8192, 1024, 4096, 1024, 24, 2048)


def check_case(oracle, name):
    from oracle import oracle_np
    case = tc.get_case(name)
    tp = np.asarray(case.term_ptr, dtype=np.int64)
    assert tp[0] == 0 and tp[-1] == len(case.post_doc) == len(case.tf) and case.tf.dtype == np.float32
    reached, detail = tc.paths(case.n_docs, case.term_ptr, case.post_doc, case.options)
    assert case.expect_paths, name
    assert case.expect_paths <= reached, (name, sorted(case.expect_paths - reached))
    assert not reached & set(tc.IMPOSSIBLE_PATHS)

    idf, (w1, m1), (w2, m2) = tc.expected(case, oracle.tfidf)
    # two restatements, one idf
    def np_tfidf(term_ptr, post_doc, tf, total_docs, n_docs):
        c_idf = oracle.tfidf(term_ptr, post_doc, tf, total_docs, n_docs)[2]
        w, mag, _ = oracle_np.tfidf(term_ptr, post_doc, tf, total_docs, n_docs, idf=c_idf)
        return w, mag, c_idf
    _, (nw1, nm1), (nw2, nm2) = tc.expected(case, np_tfidf)
    for got, want, what in ((nw1, w1, "w1"), (nm1, m1, "mag1"), (nw2, w2, "w2"), (nm2, m2, "mag2")):
        assert same_bits_or_nan(got, want), (name, what)

    # exactness of both builds
    n_nonfinite = 0
    for rnd, (w, mag) in enumerate(((w1, m1), (w2, m2))):
        ok, nonfinite, exact = tc.exactness(case.n_docs, case.post_doc, w)
        assert ok.all(), (name, rnd, np.nonzero(~ok)[0][:5])
        fin = ~nonfinite
        assert np.array_equal(bits(np.sqrt(exact[fin])), bits(mag[fin])), (name, rnd)       # the oracle's own sum is that exact sum
        assert not np.isfinite(mag[nonfinite]).any()
        n_nonfinite += int(nonfinite.sum())
        if len(case.post_doc) <= 50000:
            ok_f, nonfinite_f, f64 = tc.exactness(case.n_docs, case.post_doc, w, use_fraction=True)
            assert ok_f.all() and np.array_equal(nonfinite_f, nonfinite) and np.array_equal(f64[fin], exact[fin]), (name, rnd)
    assert (n_nonfinite > 0) == (name in tc.NONFINITE_CASES), (name, n_nonfinite)
    if name in tc.NONFINITE_CASES:
        per_doc = np.bincount(np.asarray(case.post_doc, dtype=np.int64), minlength=case.n_docs)
        assert per_doc.max() == 1                                            # no sum in the case has an order

    if name.startswith("F."):
        reached |= tc.value_paths(case, w1, idf, detail["head_terms"])
    if name == "M.many_heads":
        lens = np.diff(tp)
        assert detail["head_level"] == 1 and int((lens >= 16385).sum()) == 1100 > tc.HEAD_CAP
        assert detail["head_terms"] == np.nonzero(lens >= 32770)[0].tolist() and len(detail["head_terms"]) == 100
    kinds = {}
    for c in detail.get("chunks", []):
        kinds[c["kind"]] = kinds.get(c["kind"], 0) + 1
    print(f"{name}: P={len(case.post_doc)} T={len(tp) - 1} " +
          " ".join(f"{k}={detail[k]}" for k in ("shift", "nb", "bpt", "per", "nblk", "head_thr", "head_level") if k in detail) +
          f" heads={len(detail.get('head_terms', []))} chunks={kinds} behind_window={detail.get('n_global_search', 0)}"
          f" largest_window={max((c.get('window', 0) for c in detail.get('chunks', [])), default=0)}")
    _REACHED[name] = reached
    return reached


@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_case_reaches_its_paths_and_sums_exactly(oracle, name):
    check_case(oracle, name)


def test_every_path_has_a_case(oracle):
    """No case is left out (the GPU test parametrises over the same CASE_NAMES) and no claimed path is left without a case."""
    for name in tc.CASE_NAMES:
        if name not in _REACHED:                                             # (this test run alone, or deselected cases)
            check_case(oracle, name)
    assert set(_REACHED) == set(tc.CASE_NAMES)
    claimed = {}
    for name in tc.CASE_NAMES:
        for p in tc.get_case(name).expect_paths:
            claimed.setdefault(p, []).append(name)
    by_value = {}
    for name, reached in _REACHED.items():
        for p in reached & set(tc.REQUIRED_VALUE_PATHS):
            by_value.setdefault(p, []).append(name)
    for p in tc.REQUIRED_PATHS:
        print(f"{p}: {', '.join(claimed.get(p, []))}")
    for p in tc.REQUIRED_VALUE_PATHS:
        print(f"{p}: {', '.join(by_value.get(p, []))}")
    assert not [p for p in tc.REQUIRED_PATHS if p not in claimed]
    assert not [p for p in tc.REQUIRED_VALUE_PATHS if p not in by_value]
    assert set(claimed) <= set(tc.REQUIRED_PATHS), sorted(set(claimed) - set(tc.REQUIRED_PATHS))
    # the sizes the suite is named after
    assert [n for n in tc.CASE_NAMES if n.startswith("A.P")] == ["A.P1", "A.P8191", "A.P8192", "A.P8193", "A.P24576", "A.P8193.tight"]
    h = tc.get_case("H.heads")
    lens = np.diff(np.asarray(h.term_ptr, dtype=np.int64)).tolist()
    assert 16385 in lens and 16384 in lens and lens.index(16384) == lens.index(16385) + 1


def test_edge_values_are_what_they_are_called():
    f = tc.EDGE_TF
    tiny = np.finfo(np.float32).tiny
    assert f.dtype == np.float32 and (f == 0).sum() == 2 and np.signbit(f[1]) and not np.signbit(f[0])
    assert ((f != 0) & (np.abs(f) < tiny)).sum() >= 3 and np.float32(1e-45) == np.float32(2.0 ** -149)
    assert np.isfinite(f).all()
