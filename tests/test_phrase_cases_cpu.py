"""CPU side of the phrase-edge suite (tests/phrase_cases.py).

  * The C oracle's orc_phrase equals tests/phrase_model.py, a second restatement of retrieval/phrase.go written from the Go text
    alone, on every case and every query: docs, both float32 sums bit for bit, flags.  tests/test_gpu_phrase_edges.py compares
    the kernels with the model; this test ties the model to the oracle every other phrase test uses.
  * Every case hits the condition it is named for, proven from the model and the tables alone: the driver term and its list
    lengths (family A), a part whose close-up source and destination overlap by exactly the intended gap (B), pass-1 matches
    beyond the first workgroup part and docs that hold the driver in both fields (C), the hand-derived per-doc truth values
    (D, E, F), float32 sums that depend on the phrase order (F).
  * No case and no family is left out: the last test counts what ran.
"""
import numpy as np
import pytest

from tests import phrase_cases as pc
from tests import phrase_model

_CHECKED = {}           # case name -> number of claims checked (read by test_every_family_checked)


def f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_result(got, want, what):
    assert got[0].dtype == np.uint32 and want[0].dtype == np.uint32
    assert got[0].tolist() == want[0].tolist(), what
    assert np.array_equal(f32_bits(got[1]), f32_bits(want[1])), (what, "title")
    assert np.array_equal(f32_bits(got[2]), f32_bits(want[2])), (what, "body")
    assert got[3].tolist() == want[3].tolist(), (what, "flags")


def flags_by_doc(result):
    return {int(d): int(f) for d, f in zip(result[0], result[3])}


def field_sum(case, field, doc, phrase):
    """float32 sum of the doc's weights of the phrase terms in one table, in phrase order."""
    ptr, docs, w = case.title if field == pc.TITLE else case.body
    s = np.float32(0.0)
    for t in phrase:
        lo, hi = int(ptr[t]), int(ptr[t + 1])
        j = lo + int(np.searchsorted(docs[lo:hi], doc))
        assert j < hi and int(docs[j]) == doc
        s = np.float32(s + w[j])
    return s


def check_claim(case, q, res):
    """-> the number of conditions asserted for this query."""
    c = q.claim
    fam = c["family"]
    docs, ts, bs, flags = res
    n = 0
    if "driver" in c:
        slot, term, nb, nt = case.driver(q.phrase)
        assert (term, slot) == (c["driver"], c["slot"]), (q.name, term, slot)
        if "body_len" in c:
            assert (nb, nt) == (c["body_len"], c["title_len"]), (q.name, nb, nt)
        n += 1
    if "n_match" in c:
        assert len(docs) == c["n_match"], (q.name, len(docs))
        n += 1
    if "flags" in c:
        want = {d: f for d, f in c["flags"].items() if f}
        assert flags_by_doc(res) == want, q.name
        n += 1
    if fam == "A":
        runs = [r for r in case.runs(q.phrase) if r["pas"] == 0 and r["kind"] == "body"]
        assert len(runs) == -(-c["body_len"] // pc.PH_PART) and sum(r["n"] for r in runs) == c["n_match"], q.name
        n += 1
    if fam == "B":
        runs = [r for r in case.runs(q.phrase) if r["pas"] == 0 and r["kind"] == "body"]
        assert len(runs) == c["body_len"] // pc.PH_PART >= 2
        g = c["gap"]
        assert all(r["gap"] == g for r in runs[1:]) and runs[0]["gap"] == 0, (q.name, [r["gap"] for r in runs])
        assert all(r["n"] == pc.PH_PART for r in runs[1:]), q.name
        overlap = [r for r in runs if 0 < r["gap"] < r["n"]]
        print(f"{q.name}: parts {[(r['n'], r['gap']) for r in runs]} (matches, src - dst); overlapping moves: {len(overlap)}")
        if c["pattern"] == "allfull":
            assert g == 0 and not overlap                        # src == dst everywhere: nothing moves
        elif c["pattern"] == "part0empty":
            assert g == pc.PH_PART == runs[1]["n"] and runs[0]["n"] == 0        # gap == n: the ranges touch, no overlap
        else:
            assert g in pc.B_GAPS and len(overlap) == len(runs) - 1
        n += 1
    if fam == "C":
        drv_t = case.title[1][int(case.title[0][c["driver"]]):int(case.title[0][c["driver"] + 1])].astype(np.int64)
        drv_b = case.body[1][int(case.body[0][c["driver"]]):int(case.body[0][c["driver"] + 1])].astype(np.int64)
        fl = flags_by_doc(res)
        late = [int(d) for d in drv_t[pc.PH_PART + 1:] if fl.get(int(d), 0) & 1 and int(d) not in set(drv_b.tolist())]
        assert late, q.name                                      # a pass-1 match beyond candidate 8192 of the title list
        assert len(set(drv_t.tolist()) - set(drv_b.tolist())) > pc.PH_PART
        both = set(drv_t.tolist()) & set(drv_b.tolist())
        if c["both_fields"]:
            assert both and set(drv_b.tolist()) - both and any(fl.get(d, 0) == 3 for d in both), q.name
            assert any(fl.get(d, 0) == 0 for d in both)          # ... and docs of both lists that pass 1 must not resurrect
        else:
            assert len(drv_b) == 0
        runs = case.runs(q.phrase)
        assert sum(1 for r in runs if r["pas"] == 1) == 2 * -(-len(drv_t) // pc.PH_PART)
        print(f"{q.name}: pass-1 matches beyond candidate {pc.PH_PART}: {len(late)}; driver docs in both fields: {len(both)}")
        n += 1
    if fam == "D":
        for d, f in c["flags"].items():                          # a record carries its own field's weights only, in phrase order
            j = docs.tolist().index(d) if f else None
            if f & 1:
                assert f32_bits(ts[j]) == f32_bits(field_sum(case, pc.TITLE, d, q.phrase)), (q.name, d)
            if f & 2:
                assert f32_bits(bs[j]) == f32_bits(field_sum(case, pc.BODY, d, q.phrase)), (q.name, d)
        assert {0, 1, 2, 3} == set(c["flags"].values())
        n += 1
    if c.get("order"):
        n += 1                                                   # (the three orders are compared in test_sum_order_is_visible)
    if c.get("unknown"):
        assert len(docs) == 0 and case.driver(q.phrase) is None
        n += 1
    return n


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_oracle_equals_model_and_claims_hold(oracle, name):
    case = pc.get_case(name)
    n_claims = 0
    assert case.queries
    for q in case.queries:
        if not len(q.phrase):
            assert case.extra(q) is None
            n_claims += 1
            continue
        res = case.model_phrase(q.phrase)
        got = oracle.phrase(case.title, case.body, case.tpos, case.bpos, q.phrase)
        assert_same_result(got, res, q.name)
        k = check_claim(case, q, res)
        assert k > 0, q.name
        n_claims += k
    for q in case.errors:
        assert len(q.phrase) == pc.PH_MAX + 1 and q.claim["code"] == 7
        n_claims += 1
    _CHECKED[name] = n_claims


def test_model_module_function_is_the_class(oracle):
    case = pc.get_case("E.positions")
    q = case.queries[1]
    assert_same_result(phrase_model.phrase(case.title, case.body, case.tpos, case.bpos, q.phrase), case.model_phrase(q.phrase), q.name)


def test_sum_order_is_visible():
    """2^24 + 1 + 1 in float32 is 2^24 when the large weight comes first or second, 2^24 + 2 when it comes last: a sum that does
    not follow the phrase order gives other bits."""
    case = pc.get_case("F.lengths")
    sums = {}
    for q in case.queries:
        if q.claim.get("order"):
            docs, ts, bs, flags = case.model_phrase(q.phrase)
            assert len(docs) == 5 and (flags == 3).all() and len(set(ts.tolist())) == 1 and ts.tolist() == bs.tolist()
            sums[q.name.split(".")[-1]] = float(ts[0])
    print(f"float32 sums of the weights 2^24, 1, 1 in phrase order: {sums}")
    assert sums == {"xyz": 2.0 ** 24, "yzx": 2.0 ** 24 + 2, "zxy": 2.0 ** 24}
    assert len(set(sums.values())) >= 2
    assert {q.claim["slot"] for q in case.queries if q.claim.get("order")} == {0, 1, 2}      # the driver stands in every slot once


def test_situations_cover_the_position_edges():
    names = {s[0] for s in pc.SITUATIONS}
    assert {"empty0", "anchors", "anchor_chain", "unsorted", "duplicates", "long_last", "p24_rounds", "p25_same", "p25_plus4"} <= names
    sit = {s[0]: s for s in pc.SITUATIONS}
    assert all(len(p) >= 299 for p in sit["long_last"][1])
    assert sit["anchors"][2][1] is False and sit["anchor_chain"][2][1] is True and sit["p25_same"][2][1] is True
    case = pc.get_case("E.positions")
    for q in case.queries[:3]:                                   # every truth value occurs for the 2- and 3-term phrases
        assert {0, 1, 2, 3} >= set(q.claim["flags"].values())
    assert {1, 2} <= set(case.queries[1].claim["flags"].values()) | {3} and 0 in case.queries[1].claim["flags"].values()


def test_every_family_checked(oracle):
    """The cap against hiding: every case of the list went through the comparison and the claim check above, every family A-G
    has cases.  The GPU test parametrises over the same pc.CASE_NAMES and loops over every query of a case, as this one does."""
    for name in pc.CASE_NAMES:
        if name not in _CHECKED:                                  # (this test run alone, or deselected cases)
            test_oracle_equals_model_and_claims_hold(oracle, name)
    assert set(_CHECKED) == set(pc.CASE_NAMES)
    for fam in pc.FAMILIES:
        cases = [n for n in pc.CASE_NAMES if n[0] == fam]
        assert cases and all(_CHECKED[n] > 0 for n in cases), fam
    assert [n for n in pc.CASE_NAMES if n[0] == "A"] == [f"A.L{L}" for L in (1, 255, 256, 257, 8191, 8192, 8193, 16384, 16385)]
    assert [n for n in pc.CASE_NAMES if n[0] == "B"] == ["B.L16384", "B.L24576"]
    assert {q.claim["pattern"] for q in pc.get_case("A.L8193").queries} == {"all", "first", "last", "verylast", "none"}
    g = pc.get_case("G.batch")
    fams = {q.claim["family"] for q in g.queries}
    assert fams == set("ABCDEFG") and g.errors
    names = [tuple(q.phrase) for q in g.queries if len(q.phrase)]
    assert len(names) > len(set(names))                          # the same phrase twice
    assert any(not len(q.phrase) for q in g.queries) and any(q.claim.get("unknown") for q in g.queries)
    n_parts = set()
    for q in g.queries:
        drv = g.driver(q.phrase) if len(q.phrase) else None
        n_parts.add(0 if drv is None else -(-drv[2] // pc.PH_PART) + -(-drv[3] // pc.PH_PART))
    assert {0, 1, 2, 3} <= n_parts, n_parts                       # the part counts differ from query to query
