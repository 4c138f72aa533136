"""GPU parity: ss_field_stats and ss_field_histogram vs the model of the header's definitions (tests/field_stats_model.py) and vs the calls
that see the same docs (ss_facet_counts, ss_field_topk).  The index is test_gpu_field_topk's: two full doc blocks plus a short one whose
last word is partial, so a query has block seams and, with option "fstats.runs" at 1, 2 and 3, a run seam at neither, one or both of them.
Every histogram runs on both counting paths where the bin count admits both ("fstats.lds_bins" at 0 and 8192).  Host outputs equal the
model's bytes inside 0xA5-filled arrays one row longer than asked; device outputs equal the host bytes."""
import itertools

import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine
from tests import field_stats_model as sm
from tests.test_gpu_field_topk import (CONSTRAINT_QUERIES, F_EDGE, F_FALLING, F_RISING, F_TIES, LAST, N_DOCS, SEAMS, constraint_cases, filled,
                                       make_world)
from tests.test_gpu_group_topk import QUERIES
from tests.test_gpu_query_constraints import pack_pairs
from tests.test_gpu_score import close_all, make_scorer

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = 1, 6, 7
FILL = 0xA5
I64_MIN, I64_MAX, U64_MAX = sm.I64_MIN, sm.I64_MAX, 2 ** 64 - 1
NO_VALUE = sm.NO_VALUE
UNKNOWN = 0xFFFFFFFF
MAX_BINS = sm.MAX_HIST_BINS
ST, HT = sm.FIELD_STAT_DTYPE, sm.HIST_TAIL_DTYPE
RUNS = (0, 1, 2, 3)              # option "fstats.runs": the plan's choice, one run, a seam inside, a run per block
HIST_RUNS = (0, 1, 3)
LDS = (None, 0, 8192)            # option "fstats.lds_bins": the default, never, whenever the histogram holds the bins
OPTIONS = ("fstats.runs", "fstats.lds_bins", "fstats.scratch_bytes", "fstats.plain_divide")


@pytest.fixture(scope="module")
def world():
    return make_world()


@pytest.fixture(scope="module")
def shared_scorer(ss_ctx, world):
    sc, ti, bi = make_scorer(ss_ctx, N_DOCS, world["title"], world["body"], np.ones(N_DOCS), np.ones(N_DOCS))
    sc.set_doc_fields(world["values"])
    sc.set_doc_masks(world["words"])
    yield sc
    close_all(sc, ti, bi)


@pytest.fixture()
def scorer(ss_ctx, shared_scorer):
    yield shared_scorer
    for name in OPTIONS:
        ss_ctx.set_option(name, None)


def call_kw(mask_id=None, req=None, exc=None, clauses=None):
    return dict(ranges=None if clauses is None else engine.pack_doc_ranges(clauses), req=None if req is None else pack_pairs(req),
                exc=None if exc is None else pack_pairs(exc), mask_id=mask_id)


def model_kw(world, values, mask_id=None, req=None, exc=None, clauses=None):
    ranges = None if clauses is None else (engine.pack_doc_ranges(clauses)[0], [c for cs in clauses for c in cs])
    return dict(masks=sm.fm.unpack_masks(world["words"], N_DOCS), mask_id=mask_id, req=None if req is None else pack_pairs(req),
                exc=None if exc is None else pack_pairs(exc), ranges=ranges)


def device_like(arrays):
    import torch
    dev = [torch.full((a.nbytes,), FILL, dtype=torch.uint8, device="cuda") for a in arrays]
    torch.cuda.synchronize()
    return dev


def check_stats(ss_ctx, sc, world, queries, fields, runs=RUNS, values=None, **cons):
    """for every forced number of runs: host outputs equal the model's bytes, untouched past the last row; device outputs equal the host
    bytes; -> the model's (stats, n_match, sets)"""
    values = world["values"] if values is None else values
    n_q, n_f = len(queries), len(fields)
    assert n_q <= 14
    q_ptr, q_terms = pack_pairs(queries)
    want = sm.field_stats(N_DOCS, world["title"][:2], world["body"][:2], q_ptr, q_terms, values, fields, **model_kw(world, values, **cons))
    exp = (filled((n_q + 1, n_f), ST), filled(n_q + 1, np.uint32))
    exp[0][:n_q], exp[1][:n_q] = want[0], want[1]
    kw = call_kw(**cons)
    for r in runs:
        ss_ctx.set_option("fstats.runs", r)
        out = (filled((n_q + 1, n_f), ST), filled(n_q + 1, np.uint32))
        sc.field_stats(q_ptr, q_terms, fields, out=out, **kw)
        for name, g, w in zip(("stats", "n_match"), out, exp):
            assert g.tobytes() == w.tobytes(), (r, name, g.reshape(-1)[:4], w.reshape(-1)[:4])
        dev = device_like(out)
        sc.field_stats(q_ptr, q_terms, fields, out=tuple(dev), **kw)
        ss_ctx.synchronize()
        for name, d, h in zip(("stats", "n_match"), dev, out):
            assert d.cpu().numpy().tobytes() == h.tobytes(), (r, name)
    ss_ctx.set_option("fstats.runs", None)
    return want


def check_hist(ss_ctx, sc, world, queries, field, n_bins, origin=0, width=1, edges=None, runs=HIST_RUNS, lds=LDS, divide=(0,), **cons):
    """for every forced number of runs and both counting paths: as check_stats; -> the model's (counts, tails, sets)"""
    n_q = len(queries)
    assert n_q <= 14
    q_ptr, q_terms = pack_pairs(queries)
    want = sm.field_histogram(N_DOCS, world["title"][:2], world["body"][:2], q_ptr, q_terms, world["values"], field, n_bins, origin, width, edges,
                              **model_kw(world, world["values"], **cons))
    assert all(int(want[0][q].sum()) + sum(want[1][q].tolist()[:3]) == int(want[1][q]["n_match"]) for q in range(n_q))
    exp = (filled((n_q + 1, n_bins), np.uint32), filled(n_q + 1, HT))
    exp[0][:n_q], exp[1][:n_q] = want[0], want[1]
    kw = call_kw(**cons)
    if n_bins > 8192:
        lds = (None,)                                                          # the global path only
    for r, l, dv in itertools.product(runs, lds, divide):
        ss_ctx.set_option("fstats.runs", r)
        ss_ctx.set_option("fstats.lds_bins", l)
        ss_ctx.set_option("fstats.plain_divide", dv)
        out = (filled((n_q + 1, n_bins), np.uint32), filled(n_q + 1, HT))
        sc.field_histogram(q_ptr, q_terms, field, n_bins, origin, width, edges, out=out, **kw)
        for name, g, w in zip(("counts", "tails"), out, exp):
            assert g.tobytes() == w.tobytes(), (r, l, dv, name, g.reshape(-1)[:16], w.reshape(-1)[:16])
        dev = device_like(out)
        sc.field_histogram(q_ptr, q_terms, field, n_bins, origin, width, edges, out=tuple(dev), **kw)
        ss_ctx.synchronize()
        for name, d, h in zip(("counts", "tails"), dev, out):
            assert d.cpu().numpy().tobytes() == h.tobytes(), (r, l, dv, name)
    for name in OPTIONS:
        ss_ctx.set_option(name, None)
    return want


# ---- stats ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fields", [[F_TIES], [F_RISING], [F_FALLING], [F_EDGE], [F_TIES, F_RISING, F_FALLING, F_EDGE], [F_EDGE, F_TIES, F_EDGE]])
def test_stats(ss_ctx, world, scorer, fields):
    """every field alone, all four in one call, a repeated field; every run cut"""
    stats, n_match, sets = check_stats(ss_ctx, scorer, world, QUERIES, fields)
    assert n_match[0] > 15000 and sets[0][SEAMS].all() and n_match[8:10].tolist() == [0, 0] and n_match[10] == 2 and n_match[12] > n_match[11] > 500
    assert stats[8, 0].tolist() == (I64_MAX, I64_MIN, 0, 0, 0, 0)                # no term: the identity entry
    if F_EDGE in fields:
        e = stats[:, fields.index(F_EDGE)]
        assert e["sum_hi"].max() >= 1 and e["missing"][0] > 100 and e["min"][0] == I64_MIN + 1 and e["max"][0] == I64_MAX   # the sum leaves 64 bits
        assert (e["count"] + e["missing"] == n_match).all()
    if fields == [F_EDGE, F_TIES, F_EDGE]:
        assert stats[:, 0].tobytes() == stats[:, 2].tobytes()
    if F_RISING in fields:
        s = stats[0, fields.index(F_RISING)]
        assert s["missing"] == 0 and s["min"] == -100000 and s["max"] == 3 * LAST - 100000   # docs 0 and LAST match query 0


@pytest.mark.parametrize("table", ["max", "minus-one", "missing"])
def test_stats_of_constant_tables(ss_ctx, world, scorer, table):
    value = {"max": I64_MAX, "minus-one": -1, "missing": NO_VALUE}[table]
    values = np.full((1, N_DOCS), value, np.int64)
    try:
        scorer.set_doc_fields(values)
        stats, n_match, _ = check_stats(ss_ctx, scorer, world, QUERIES, [0], runs=(0, 3), values=values)
    finally:
        scorer.set_doc_fields(world["values"])
    s = stats[0, 0]
    if table == "max":
        assert s["sum_hi"] > 7000 and s["min"] == s["max"] == I64_MAX and s["count"] == n_match[0]
    if table == "minus-one":
        assert s["sum_hi"] == -1 and int(s["sum_lo"]) == 2 ** 64 - int(n_match[0]) and stats[10, 0].tolist() == (-1, -1, 2 ** 64 - 2, -1, 2, 0)
    if table == "missing":
        assert (stats[:, 0]["count"] == 0).all() and (stats[:, 0]["missing"] == n_match).all() and s.tolist() == (I64_MAX, I64_MIN, 0, 0, 0, int(n_match[0]))


def test_stats_agree_with_field_topk_and_facet_counts(ss_ctx, world, scorer):
    """where no value is missing, min / max are the first value of ss_field_topk ascending / descending; n_match is ss_facet_counts'"""
    fields = [F_TIES, F_RISING, F_FALLING]
    stats, n_match, _ = check_stats(ss_ctx, scorer, world, QUERIES, fields, runs=(0,))
    q_ptr, q_terms = pack_pairs(QUERIES)
    assert scorer.facet_counts(q_ptr, q_terms, want_masks=False)[0].tolist() == n_match.tolist()
    for i, f in enumerate(fields):
        for desc, name in ((False, "min"), (True, "max")):
            _, n_out, values, _ = scorer.field_topk(q_ptr, q_terms, f, desc, 0, 1)
            for q in range(len(QUERIES)):
                assert n_out[q] == (1 if n_match[q] else 0)
                if n_out[q]:
                    assert values[q, 0] == stats[q, i][name], (f, name, q)


# ---- histograms -----------------------------------------------------------------------------------------------------------------------------

FIXED = {
    "rising-30": (F_RISING, -100000, 30, 6558),            # both paths, ascending bins, the merge of equal neighbours
    "rising-6": (F_RISING, -100000, 6, 32787),             # the global path only
    "falling-30": (F_FALLING, 100001 - 30 * 6558, 30, 6558),   # the mirror: descending bins
    "ties-3": (F_TIES, 5, 1, 3),
    "ties-1": (F_TIES, 6, 1, 1),                           # below and above both non-zero
    "edge-min": (F_EDGE, I64_MIN, 1, 1),                   # INT64_MIN is missing, not bin 0
    "edge-halves": (F_EDGE, I64_MIN + 1, 2 ** 63, 2),
    "edge-max": (F_EDGE, I64_MAX, 1, 1),
    "edge-7": (F_EDGE, -1000, 7, 300),                     # a width that is no power of two: the divider
    "edge-widest": (F_EDGE, -5, U64_MAX, 3),
    "edge-widest-all": (F_EDGE, I64_MIN + 1, U64_MAX, 1),
    "rising-most-bins": (F_RISING, -100000, 2, MAX_BINS),  # SS_MAX_HIST_BINS
}


@pytest.mark.parametrize("case", list(FIXED))
def test_fixed_width(ss_ctx, world, scorer, case):
    field, origin, width, n_bins = FIXED[case]
    divide = (0, 1) if width & (width - 1) else (0,)                           # the reciprocal and `/` give the same bytes
    counts, tails, sets = check_hist(ss_ctx, scorer, world, QUERIES, field, n_bins, origin, width, divide=divide,
                                     runs=HIST_RUNS if n_bins < 30000 else (0, 3))
    t = tails[0]
    assert t["n_match"] > 15000 and tails["n_match"][8:10].tolist() == [0, 0] and counts[8:10].sum() == 0
    if case in ("rising-30", "rising-6", "falling-30"):
        assert t["below"] == t["above"] == t["missing"] == 0 and counts[0].max() <= 10 and np.count_nonzero(counts[0]) > 5000
        assert counts[0][0 if case != "falling-30" else -1] >= 1 and counts[0][-1 if case != "falling-30" else 0] >= 1   # docs 0 and LAST
    if case == "ties-3":
        assert t["below"] == t["above"] == 0 and (counts[0] > 3000).all()
    if case == "ties-1":
        assert t["below"] > 3000 and t["above"] > 3000 and counts[0][0] > 3000
    if case == "edge-min":
        assert counts[0][0] == 0 and t["below"] == 0 and t["missing"] > 100 and t["above"] == t["n_match"] - t["missing"]
    if case == "edge-halves":
        assert t["below"] == t["above"] == 0 and counts[0].min() > 3000
    if case == "edge-max":
        assert counts[0][0] > 100 and t["above"] == 0 and t["below"] > 10000
    if case == "edge-7":
        assert t["below"] > 300 and t["above"] > 300 and np.count_nonzero(counts[0]) > 250
    if case == "edge-widest":
        assert t["above"] == 0 and counts[0][0] > 3000 and counts[0][1:].sum() == 0 and t["below"] > 3000
    if case == "edge-widest-all":
        assert counts[0][0] == t["n_match"] - t["missing"]
    if case == "rising-most-bins":
        assert t["above"] > 3000 and t["below"] == 0


def edge_lists():
    rng = np.random.default_rng(9)
    days = np.array([31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31] * 20)
    months = -90000 + np.concatenate([[0], np.cumsum(days * 25)])               # 240 irregular bins, docs before the first and behind the last
    many = np.sort(rng.choice(np.arange(-100000, 97000), MAX_BINS + 1, replace=False))
    return {"months": (F_RISING, months), "one-bin": (F_TIES, [6, 7]), "most-edges": (F_RISING, many), "ends": (F_EDGE, [I64_MIN, 0, I64_MAX]),
            "lds-edges-limit": (F_RISING, np.arange(-100000, -100000 + 193 * 1025, 193)), "past-lds-edges": (F_RISING, np.arange(-100000, -100000 + 193 * 1026, 193))}


@pytest.mark.parametrize("case", list(edge_lists()))
def test_edges(ss_ctx, world, scorer, case):
    field, edges = edge_lists()[case]
    edges = np.asarray(edges, np.int64)
    n_bins = len(edges) - 1
    counts, tails, _ = check_hist(ss_ctx, scorer, world, QUERIES, field, n_bins, origin=12345, width=0, edges=edges,
                                  runs=HIST_RUNS if n_bins < 30000 else (0, 3))
    t = tails[0]
    if case == "months":
        assert n_bins == 240 and t["below"] > 100 and t["above"] > 100 and (counts[0] > 20).all()
    if case == "one-bin":
        assert t["below"] > 3000 and t["above"] > 3000 and counts[0][0] > 3000
    if case == "most-edges":
        assert n_bins == MAX_BINS and np.count_nonzero(counts[0]) > 3000
    if case == "ends":
        assert t["below"] == 0 and t["missing"] > 100 and t["above"] > 100 and counts[0].min() > 3000   # INT64_MIN is missing; INT64_MAX is above
    if case in ("lds-edges-limit", "past-lds-edges"):
        assert n_bins == (1024 if case == "lds-edges-limit" else 1025) and t["below"] == 0 and t["above"] == 0


def test_agrees_with_facet_counts_buckets(ss_ctx, world, scorer):
    """a fixed-width histogram of at most 64 bins equals ss_facet_counts with the buckets [origin + b w, origin + (b + 1) w - 1]"""
    q_ptr, q_terms = pack_pairs(QUERIES)
    for field, origin, width, n_bins in ((F_TIES, 5, 1, 3), (F_TIES, 4, 2, 2), (F_RISING, -100000, 3074, 64), (F_RISING, -50000, 1000, 40)):
        counts, tails, _ = check_hist(ss_ctx, scorer, world, QUERIES, field, n_bins, origin, width, runs=(0,), lds=(None, 0))
        buckets = [(field, origin + b * width, origin + (b + 1) * width - 1) for b in range(n_bins)]
        total, _, by_bucket = scorer.facet_counts(q_ptr, q_terms, buckets=buckets, want_masks=False)
        assert by_bucket.tolist() == counts.tolist() and total.tolist() == tails["n_match"].tolist(), (field, origin)
    assert tails["below"][0] > 1000 and tails["above"][0] > 1000


# ---- the allowed set, the scratch bound ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(constraint_cases()))
def test_constraints(ss_ctx, world, scorer, case):
    kw = constraint_cases()[case]
    stats, n_match, _ = check_stats(ss_ctx, scorer, world, CONSTRAINT_QUERIES, [F_EDGE, F_RISING], runs=(0, 1), **kw)
    counts, tails, _ = check_hist(ss_ctx, scorer, world, CONSTRAINT_QUERIES, F_RISING, 6558, -100000, 30, runs=(0, 1), lds=(None, 0), **kw)
    assert tails["n_match"].tolist() == n_match.tolist()
    q_ptr, q_terms = pack_pairs(CONSTRAINT_QUERIES)
    free = sm.field_stats(N_DOCS, world["title"][:2], world["body"][:2], q_ptr, q_terms, world["values"], [F_EDGE],
                          masks=sm.fm.unpack_masks(world["words"], N_DOCS))[1]
    assert (n_match <= free).all()
    if case != "empty-arrays":
        assert (n_match < free).any() and n_match.sum() > 0
    else:
        assert n_match.tolist() == free.tolist()
    if case == "all":
        assert n_match[-1] == 0 and free[-1] > 0 and stats[-1, 0].tolist() == (I64_MAX, I64_MIN, 0, 0, 0, 0)   # a list, but no allowed doc
    if case == "one-clause":
        assert n_match[5] == 0 and free[5] > 0


def test_groups_under_a_small_scratch_bound(ss_ctx, world, scorer):
    """a scratch bound below one query's partial entries or counter row: one query per group, the groups re-use the block in stream order"""
    ss_ctx.set_option("fstats.scratch_bytes", 1)
    check_stats(ss_ctx, scorer, world, QUERIES, [F_EDGE, F_TIES], runs=(0, 3))
    ss_ctx.set_option("fstats.scratch_bytes", 1)
    check_hist(ss_ctx, scorer, world, QUERIES, F_RISING, 6558, -100000, 30, runs=(0, 3))
    ss_ctx.set_option("fstats.scratch_bytes", 3 * 16 * ((300 + 4 + 3) // 4))    # three queries of 300 bins
    check_hist(ss_ctx, scorer, world, QUERIES, F_EDGE, 300, -1000, 7, runs=(1,))
    ss_ctx.set_option("fstats.scratch_bytes", 3 * 3 * 2 * 40)                   # three queries of three runs and two fields
    check_stats(ss_ctx, scorer, world, QUERIES, [F_EDGE, F_TIES], runs=(3,))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_outputs_untouched(ss_ctx, world, scorer):
    """invalid ARGUMENTS only: every refusal returns its code and leaves 0xA5 outputs as they were"""
    sc, lib = scorer, ss_ctx.lib
    queries = [[7, 8], [31]]
    q_ptr, q_terms = pack_pairs(queries)
    s_out = (filled((2, 4), ST), filled(2, np.uint32))
    h_out = (filled((2, 4), np.uint32), filled(2, HT))
    before = [a.tobytes() for a in s_out + h_out]
    untouched = lambda: [a.tobytes() for a in s_out + h_out] == before          # noqa: E731

    def refused(code, q_ptr=q_ptr, q_terms=q_terms, fields=(0,), field=0, n_bins=4, origin=0, width=1, edges=None, which="both", **kw):
        if which in ("both", "stats"):
            with pytest.raises(SpaghettiError) as ei:
                sc.field_stats(q_ptr, q_terms, list(fields), out=s_out, **kw)
            assert ei.value.code == code, (ei.value, kw)
        if which in ("both", "hist"):
            with pytest.raises(SpaghettiError) as ei:
                sc.field_histogram(q_ptr, q_terms, field, n_bins, origin, width, edges, out=h_out, **kw)
            assert ei.value.code == code, (ei.value, kw)
        assert untouched()

    refused(ERR_INVALID, q_ptr=np.array([0, 2, 1], np.uint32))                                   # q_ptr decreases
    refused(ERR_INVALID, mask_id=np.array([0, 3], np.int32))                                     # no such mask
    refused(ERR_INVALID, mask_id=np.array([-2, 0], np.int32))
    refused(ERR_INVALID, req=(np.array([1, 1, 1], np.uint32), np.array([7], np.uint32)))         # req_ptr does not start at 0
    refused(ERR_INVALID, exc=(np.array([0, 1, 0], np.uint32), np.array([7], np.uint32)))         # exc_ptr decreases
    refused(ERR_UNSUPPORTED, req=pack_pairs([list(range(17)), []]))                              # 17 distinct constraint terms
    refused(ERR_INVALID, ranges=engine.pack_doc_ranges([[(4, 0, 1)], []]))                       # a clause on a field that is not there
    refused(ERR_INVALID, ranges=(np.array([0, 1, 0], np.uint32), engine.pack_doc_ranges([[(0, 0, 1)]])[1]))
    refused(ERR_UNSUPPORTED, ranges=engine.pack_doc_ranges([[(0, 0, 1)] * 5, []]))               # five clauses
    refused(ERR_INVALID, fields=(), which="stats")                                               # n_stat_fields < 1
    refused(ERR_INVALID, fields=(4,), which="stats")
    refused(ERR_INVALID, fields=(0, 1, -1), which="stats")
    refused(ERR_INVALID, field=4, which="hist")
    refused(ERR_INVALID, field=-1, which="hist")
    refused(ERR_INVALID, n_bins=0, which="hist")
    refused(ERR_INVALID, width=0, which="hist")
    refused(ERR_INVALID, n_bins=2, edges=[1, 2, 2], which="hist")                                # not strictly ascending
    refused(ERR_INVALID, n_bins=2, edges=[3, 2, 4], which="hist")
    refused(ERR_INVALID, n_bins=1, edges=[I64_MAX, I64_MIN], which="hist")
    # the raw ABI: NULL pointers, negative counts and counts past the limits
    ptr = lambda a: a.ctypes.data                                                                 # noqa: E731
    five = np.zeros(5, np.int32)
    big_edges = np.arange(MAX_BINS + 2, dtype=np.int64)
    s_args = lambda **o: [o.get("s", sc.h), o.get("n_q", 2), o.get("q_ptr", ptr(q_ptr)), o.get("q_terms", ptr(q_terms)), None, None, None, None, None,   # noqa: E731
                          None, None, o.get("n", 1), o.get("fields", ptr(five)), o.get("stats", ptr(s_out[0])), ptr(s_out[1])]
    h_args = lambda **o: [o.get("s", sc.h), o.get("n_q", 2), o.get("q_ptr", ptr(q_ptr)), o.get("q_terms", ptr(q_terms)), None, None, None, None, None,   # noqa: E731
                          None, None, o.get("field", 0), 0, o.get("width", 1), o.get("edges", None), o.get("n_bins", 4), o.get("counts", ptr(h_out[0])),
                          ptr(h_out[1])]
    for code, o in ((ERR_INVALID, dict(s=None)), (ERR_INVALID, dict(n_q=-1)), (ERR_INVALID, dict(q_ptr=None)), (ERR_INVALID, dict(q_terms=None)),
                    (ERR_INVALID, dict(stats=None)), (ERR_INVALID, dict(n=0)), (ERR_INVALID, dict(n=-1)), (ERR_INVALID, dict(fields=None)),
                    (ERR_UNSUPPORTED, dict(n=5)), (ERR_UNSUPPORTED, dict(n=2 ** 31 - 1))):
        assert lib.ss_field_stats(*s_args(**o)) == code, o
        assert untouched()
    for code, o in ((ERR_INVALID, dict(s=None)), (ERR_INVALID, dict(n_q=-1)), (ERR_INVALID, dict(q_ptr=None)), (ERR_INVALID, dict(q_terms=None)),
                    (ERR_INVALID, dict(counts=None)), (ERR_INVALID, dict(n_bins=0)), (ERR_INVALID, dict(n_bins=-1)), (ERR_INVALID, dict(width=0)),
                    (ERR_UNSUPPORTED, dict(n_bins=MAX_BINS + 1)), (ERR_UNSUPPORTED, dict(n_bins=MAX_BINS + 1, edges=ptr(big_edges))),
                    (ERR_UNSUPPORTED, dict(n_bins=2 ** 31 - 1))):
        assert lib.ss_field_histogram(*h_args(**o)) == code, o
        assert untouched()
    # n_q == 0 comes first: SS_OK, nothing done
    for o in (dict(), dict(n=0), dict(n=9), dict(fields=None), dict(q_ptr=None, stats=None)):
        assert lib.ss_field_stats(*s_args(n_q=0, **o)) == 0 and untouched()
    for o in (dict(), dict(n_bins=0), dict(n_bins=MAX_BINS + 1), dict(width=0), dict(field=9), dict(q_ptr=None, counts=None)):
        assert lib.ss_field_histogram(*h_args(n_q=0, **o)) == 0 and untouched()
    try:
        sc.set_doc_fields(None)                                                                  # no field table
        refused(ERR_STATE)
        assert lib.ss_field_stats(*s_args(n_q=0)) == 0 and lib.ss_field_histogram(*h_args(n_q=0)) == 0 and untouched()
    finally:
        sc.set_doc_fields(world["values"])


def test_too_many_query_terms(ss_ctx):
    """65 distinct usable terms in one query are refused as ss_facet_counts refuses them; 64 are counted"""
    n_docs, n_terms = 40, 70
    ptr = np.arange(n_terms + 1, dtype=np.uint64)
    doc = (np.arange(n_terms) % n_docs).astype(np.uint32)
    table = (ptr, doc, np.ones(n_terms, np.float32))
    sc, ti, bi = make_scorer(ss_ctx, n_docs, table, table, np.ones(n_docs), np.ones(n_docs))
    try:
        sc.set_doc_fields(np.arange(n_docs, dtype=np.int64)[None, :] % 7)
        s_out, h_out = (filled((1, 1), ST), filled(1, np.uint32)), (filled((1, 7), np.uint32), filled(1, HT))
        before = [a.tobytes() for a in s_out + h_out]
        too_many = (np.array([0, 65], np.uint32), np.arange(65, dtype=np.uint32))
        with pytest.raises(SpaghettiError) as ei:
            sc.field_stats(*too_many, [0], out=s_out)
        assert ei.value.code == ERR_UNSUPPORTED
        with pytest.raises(SpaghettiError) as ei:
            sc.field_histogram(*too_many, 0, 7, out=h_out)
        assert ei.value.code == ERR_UNSUPPORTED and [a.tobytes() for a in s_out + h_out] == before
        most = (np.array([0, 66], np.uint32), np.concatenate([np.arange(64), [0, UNKNOWN]]).astype(np.uint32))
        stats, n_match = sc.field_stats(*most, [0])
        assert n_match.tolist() == [40] and stats[0, 0].tolist() == (0, 6, sum(d % 7 for d in range(40)), 0, 40, 0)
        counts, tails = sc.field_histogram(*most, 0, 7)
        assert counts[0].tolist() == [6, 6, 6, 6, 6, 5, 5] and tails[0].tolist() == (0, 0, 0, 40)
    finally:
        close_all(sc, ti, bi)
