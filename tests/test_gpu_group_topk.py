"""GPU parity: ss_top_groups and ss_scorer_group_values vs the model of the header's definition (tests/group_topk_model.py) and vs
ss_facet_counts, which sees the same docs.  The index is test_gpu_field_topk's: two full doc blocks of k_group_count plus a short one
whose last word is partial, so a query has block seams and, with option "gtopk.runs" at 1 and 3, runs of three blocks (bounds searched
warm from the previous block's ends) and of one.  Every case runs on both counting paths where the table admits both ("gtopk.lds_groups"
at 0 and above the table's distinct values).  Rows, n_out, n_groups, n_ungrouped and n_match equal the model's byte for byte; host
outputs start from 0xA5 bytes and are one row longer than asked, so an entry the call must not write is checked with the ones it must;
device outputs equal the host bytes."""
import itertools

import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine
from tests import group_topk_model as gm
from tests.test_gpu_field_topk import (BLOCK, BOTH, CONSTRAINT_QUERIES, LAST, MIXED, N_DOCS, N_TERMS, SEAMS, constraint_cases, filled,
                                       make_world)
from tests.test_gpu_query_constraints import pack_pairs
from tests.test_gpu_score import close_all, make_scorer

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = 1, 6, 7
FILL = 0xA5
MAX_TOPK = 1024
UNKNOWN = 0xFFFFFFFF
NO_GROUP = gm.NO_GROUP
GC = gm.GROUP_COUNT_DTYPE
RUNS = (0, 1, 3)                 # option "gtopk.runs": the plan's choice, one run of three blocks, a run per block
LDS = (None, 0, 100000)          # option "gtopk.lds_groups": the default, never, whenever the histogram holds the table
OPTIONS = ("gtopk.runs", "gtopk.lds_groups", "gtopk.scratch_bytes")
NAMES = ("groups", "n_out", "n_groups", "n_ungrouped", "n_match")


def make_tables():
    rng = np.random.default_rng(77)
    five = np.array([0, 5, 1000, 0x80000000, 0xFFFFFFFE], np.uint32)
    a = five[rng.choice(5, N_DOCS, p=[0.4, 0.3, 0.15, 0.1, 0.05])]
    a[rng.random(N_DOCS) < 0.25] = NO_GROUP
    a[SEAMS] = [0, 5, 0xFFFFFFFE, NO_GROUP, 0x80000000, 0xFFFFFFFE]
    b = (np.arange(N_DOCS, dtype=np.uint64) * 65521 % (2 ** 32 - 1)).astype(np.uint32)          # every doc a group of its own, not in doc order
    assert len(np.unique(b)) == N_DOCS and NO_GROUP not in b
    c = np.full(N_DOCS, 42, np.uint32)
    lens = rng.integers(1, 41, N_DOCS)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), N_DOCS)) + 1]
    sites = (rng.permutation(len(lens)).astype(np.uint64) % 3000 * 2654435761 % (2 ** 32 - 1)).astype(np.uint32)   # 3000 hashed values, some in two runs
    d = np.repeat(sites, lens)[:N_DOCS].copy()
    d[rng.random(N_DOCS) < 0.02] = NO_GROUP                                                     # holes inside the clusters
    e = (np.arange(N_DOCS) % 50 * 3).astype(np.uint32)                                          # 50 groups of equal size: counts tie
    return {"a": a, "b": b, "c": c, "d": d, "e": e}


@pytest.fixture(scope="module")
def world():
    w = make_world()
    w["tables"] = make_tables()
    return w


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


def model(world, group, queries, first, m, mask_id=None, req=None, exc=None, clauses=None):
    q_ptr, q_terms = pack_pairs(queries)
    ranges = None if clauses is None else (engine.pack_doc_ranges(clauses)[0], [c for cs in clauses for c in cs])
    return gm.top_groups(N_DOCS, world["title"][:2], world["body"][:2], q_ptr, q_terms, group, first, m,
                         masks=gm.fm.unpack_masks(world["words"], N_DOCS), fields=world["values"], mask_id=mask_id,
                         req=None if req is None else pack_pairs(req), exc=None if exc is None else pack_pairs(exc), ranges=ranges)


def fresh(n_q, m):
    return (filled((n_q + 1, m), GC), filled(n_q + 1, np.int32), filled(n_q + 1, np.uint32), filled(n_q + 1, np.uint32), filled(n_q + 1, np.uint32))


def expected(want, n_q, m):
    """the model's pages inside 0xA5 arrays of one row more than asked"""
    exp = fresh(n_q, m)
    for q in range(n_q):
        exp[0][q, :len(want[0][q])] = want[0][q]
    for a, w in zip(exp[1:], want[1:5]):
        a[:n_q] = w
    return exp


def check(ss_ctx, sc, world, table, queries, first=0, m=10, runs=RUNS, lds=LDS, mask_id=None, req=None, exc=None, clauses=None):
    """registers the table; for every forced number of runs and both counting paths: host outputs equal the model's bytes, untouched past
    n_out[q] and past the last row; device outputs equal the host bytes; -> the model's results"""
    import torch
    group = world["tables"][table] if isinstance(table, str) else table
    sc.set_doc_groups(group)
    n_q = len(queries)
    assert n_q <= 14
    want = model(world, group, queries, first, m, mask_id, req, exc, clauses)
    exp = expected(want, n_q, m)
    q_ptr, q_terms = pack_pairs(queries)
    kw = dict(ranges=None if clauses is None else engine.pack_doc_ranges(clauses), req=None if req is None else pack_pairs(req),
              exc=None if exc is None else pack_pairs(exc), mask_id=mask_id)
    for r, l in itertools.product(runs, lds):
        ss_ctx.set_option("gtopk.runs", r)
        ss_ctx.set_option("gtopk.lds_groups", l)
        out = fresh(n_q, m)
        sc.top_groups(q_ptr, q_terms, first, m, out=out, **kw)
        for name, g, w in zip(NAMES, out, exp):
            assert g.tobytes() == w.tobytes(), (r, l, name, g.reshape(-1)[:16], w.reshape(-1)[:16])
        dev = [torch.full((a.nbytes,), FILL, dtype=torch.uint8, device="cuda") for a in out]
        torch.cuda.synchronize()
        sc.top_groups(q_ptr, q_terms, first, m, out=tuple(dev), **kw)
        ss_ctx.synchronize()
        for name, d, h in zip(NAMES, dev, out):
            assert d.cpu().numpy().tobytes() == h.tobytes(), (r, l, name)
    ss_ctx.set_option("gtopk.runs", None)
    ss_ctx.set_option("gtopk.lds_groups", None)
    return want


QUERIES = MIXED + [[], [UNKNOWN, N_TERMS], [3], BOTH, list(range(N_TERMS)), [4, 5]]       # 14: long lists, seams, no term, unknown ids only,
#                                                                                            two docs, 36 lists, every term (61 lists)


# ---- the group ranks ------------------------------------------------------------------------------------------------------------------------

def test_group_values_agree_with_unique(world, scorer):
    for name, group in world["tables"].items():
        scorer.set_doc_groups(group)
        got = scorer.group_values()
        assert got.dtype == np.uint32 and got.tobytes() == gm.group_values(group).tobytes(), name
        assert scorer.group_values().tobytes() == got.tobytes()                 # built once, read again
    sizes = {n: len(gm.group_values(g)) for n, g in world["tables"].items()}
    assert sizes["a"] == 5 and sizes["b"] == N_DOCS and sizes["c"] == 1 and 2500 < sizes["d"] <= 3000 and sizes["e"] == 50
    only_none = np.full(N_DOCS, NO_GROUP, np.uint32)
    scorer.set_doc_groups(only_none)
    assert scorer.group_values().size == 0


# ---- every table on both paths, every run cut -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table", ["a", "b", "c", "d", "e"])
def test_tables(ss_ctx, world, scorer, table):
    rows, n_out, n_groups, n_ungrouped, n_match, sets = check(ss_ctx, scorer, world, table, QUERIES, 0, 10)
    assert n_match[0] > 15000 and sets[0][SEAMS].all() and n_match[8:10].tolist() == [0, 0] and n_match[10] == 2 and n_match[12] > n_match[11] > 500
    if table == "a":
        assert n_groups[0] == 5 and n_ungrouped[0] > 3000 and {0, 0xFFFFFFFE} <= set(rows[0]["group"].tolist())
    if table == "b":
        assert n_groups.tolist() == n_match.tolist() and n_ungrouped.sum() == 0 and n_groups[0] > MAX_TOPK
        assert (rows[0]["count"] == 1).all() and (np.diff(rows[0]["group"].astype(np.int64)) > 0).all()   # all tie: value ascending
    if table == "c":
        assert n_groups[:8].tolist() == [1] * 8 and rows[0].tolist() == [(42, int(n_match[0]))]
    if table == "d":
        assert n_groups[0] > 1500 and rows[0]["count"][0] > 5 and 0 < n_ungrouped[0] < n_match[0]
    if table == "e":
        assert n_groups[0] == 50 and sum(len(r) - len(set(r["count"].tolist())) for r in rows) > 10   # groups tie in count inside the pages


def test_no_group_anywhere(ss_ctx, world, scorer):
    """a table of SS_NO_GROUP only: no counter, every match ungrouped"""
    _, n_out, n_groups, n_ungrouped, n_match, _ = check(ss_ctx, scorer, world, np.full(N_DOCS, NO_GROUP, np.uint32), QUERIES[:6], 0, 3)
    assert n_out.sum() == 0 and n_groups.sum() == 0 and n_ungrouped.tolist() == n_match.tolist() and n_match[0] > 15000


# ---- pages ----------------------------------------------------------------------------------------------------------------------------------

def test_pages(ss_ctx, world, scorer):
    queries = [[36], [7], [0, 1], [], [3], [31, 7], [UNKNOWN, N_TERMS]]
    _, n_out, n_groups, _, _, _ = check(ss_ctx, scorer, world, "a", queries, 0, 1)
    assert n_out.tolist() == [1, 1, 1, 0, 1, 1, 0]
    _, n_out, _, _, _, _ = check(ss_ctx, scorer, world, "a", queries, 5, 7, runs=(0,))          # first at / past the last group
    assert n_out.sum() == 0 and n_groups[0] == 5
    _, n_out, _, _, _, _ = check(ss_ctx, scorer, world, "a", queries, 3, 40, runs=(3,))          # m larger than n_groups
    assert n_out[0] == 2
    rows, n_out, n_groups, _, _, _ = check(ss_ctx, scorer, world, "e", queries, 0, MAX_TOPK, runs=(1,))
    assert n_out[0] == n_groups[0] == 50
    # more than SS_MAX_TOPK matched groups, first + m = SS_MAX_TOPK: the buffer is compacted again and again
    rows, n_out, n_groups, _, _, _ = check(ss_ctx, scorer, world, "b", queries, 1000, 24, lds=(None,))
    assert n_groups[0] > 15000 and n_out.tolist() == [24, 0, 0, 0, 0, 24, 0]
    rows, n_out, _, _, _, _ = check(ss_ctx, scorer, world, "b", queries, 0, MAX_TOPK, runs=(0, 3), lds=(None,))
    assert n_out[0] == MAX_TOPK and n_out[2] == 9
    rows, n_out, n_groups, _, _, _ = check(ss_ctx, scorer, world, "d", queries, 1000, 24, runs=(0,))
    assert n_groups[0] > 1024 and n_out[0] == 24


# ---- the allowed set ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(constraint_cases()))
def test_constraints(ss_ctx, world, scorer, case):
    """a mask, required terms, excluded terms, one and four range clauses, all together (with a term required AND excluded and a clause
    with lo > hi: empty allowed sets), one set shared by every query, empty constraint arrays"""
    kw = constraint_cases()[case]
    table = "d" if case in ("mask", "all", "shared-set") else "a"
    _, _, _, n_ungrouped, n_match, _ = check(ss_ctx, scorer, world, table, CONSTRAINT_QUERIES, 0, 30, runs=(0, 1), lds=(None, 0), **kw)
    free = model(world, world["tables"][table], CONSTRAINT_QUERIES, 0, 30)[4]
    assert (n_match <= free).all()
    if case != "empty-arrays":
        assert (n_match < free).any() and n_match.sum() > 0
    else:
        assert n_match.tolist() == free.tolist()
    if case == "all":
        assert n_match[-1] == 0 and free[-1] > 0
    if case == "one-clause":
        assert n_match[5] == 0 and free[5] > 0


def test_groups_under_a_small_scratch_bound(ss_ctx, world, scorer):
    """a scratch bound below one query's counter row: one query per group, the groups re-use the rows in stream order"""
    ss_ctx.set_option("gtopk.scratch_bytes", 1)
    check(ss_ctx, scorer, world, "b", QUERIES, 2, 100, runs=(0, 3))              # a row of 65575 counters against a bound of one byte
    check(ss_ctx, scorer, world, "d", QUERIES, 0, 20, runs=(1,))
    ss_ctx.set_option("gtopk.scratch_bytes", 3 * 16 * ((5 + 2 + 3) // 4))        # three queries of table a
    check(ss_ctx, scorer, world, "a", QUERIES, 0, 5, runs=(0,))


# ---- agreement with ss_facet_counts -----------------------------------------------------------------------------------------------------------

def test_agrees_with_facet_counts(ss_ctx, world, scorer):
    """n_match = ss_facet_counts' totals; with a group's docs registered as an allow-list, that list's count is the group's; the counts
    of all groups plus n_ungrouped add up to n_match"""
    sc = scorer
    group = world["tables"]["a"]
    queries = QUERIES[:8] + [[3], [4, 5]]
    req = [[31]] + [[] for _ in queries[1:]]
    rows, n_out, n_groups, n_ungrouped, n_match, _ = check(ss_ctx, sc, world, "a", queries, 0, 8, runs=(0,), req=req)
    q_ptr, q_terms = pack_pairs(queries)
    values = gm.group_values(group)
    try:
        sc.set_doc_masks(engine.pack_doc_masks(np.stack([group == v for v in values]), N_DOCS))
        total, by_mask, _ = sc.facet_counts(q_ptr, q_terms, req=pack_pairs(req))
    finally:
        sc.set_doc_masks(world["words"])
    assert total.tolist() == n_match.tolist()
    for q in range(len(queries)):
        assert n_out[q] == n_groups[q] <= 5
        assert {int(g): int(c) for g, c in rows[q].tolist()} == {int(v): int(c) for v, c in zip(values, by_mask[q]) if c}
        assert int(rows[q]["count"].sum()) + int(n_ungrouped[q]) == int(n_match[q])
    assert n_match[0] > 500 and n_ungrouped[0] > 100


def test_registering_again_and_clearing(ss_ctx, world, scorer):
    sc = scorer
    first = check(ss_ctx, sc, world, "a", QUERIES[:4], 0, 6, runs=(0,))
    second = check(ss_ctx, sc, world, "e", QUERIES[:4], 0, 6, runs=(0,))        # the ranks of table a are dropped with it
    assert first[0][0].tolist() != second[0][0].tolist() and first[4].tolist() == second[4].tolist()
    again = check(ss_ctx, sc, world, "a", QUERIES[:4], 0, 6, runs=(0,))
    assert again[0][0].tolist() == first[0][0].tolist()
    sc.set_doc_groups(None)
    out = fresh(4, 6)
    before = [a.tobytes() for a in out]
    q_ptr, q_terms = pack_pairs(QUERIES[:4])
    with pytest.raises(SpaghettiError) as ei:
        sc.top_groups(q_ptr, q_terms, 0, 6, out=out)
    assert ei.value.code == ERR_STATE and [a.tobytes() for a in out] == before
    with pytest.raises(SpaghettiError) as ei:
        sc.group_values()
    assert ei.value.code == ERR_STATE


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_outputs_untouched(ss_ctx, world, scorer):
    """invalid ARGUMENTS only: every refusal returns its code and leaves 0xA5 outputs as they were"""
    sc, lib = scorer, ss_ctx.lib
    sc.set_doc_groups(world["tables"]["a"])
    queries = [[7, 8], [31]]
    q_ptr, q_terms = pack_pairs(queries)
    out = fresh(1, 4)
    before = [a.tobytes() for a in out]

    def refused(code, q_ptr=q_ptr, q_terms=q_terms, first=0, m=4, **kw):
        with pytest.raises(SpaghettiError) as ei:
            sc.top_groups(q_ptr, q_terms, first, m, out=out, **kw)
        assert ei.value.code == code, (ei.value, kw)
        assert [a.tobytes() for a in out] == before

    refused(ERR_INVALID, q_ptr=np.array([0, 2, 1], np.uint32))                                   # q_ptr decreases
    refused(ERR_INVALID, mask_id=np.array([0, 3], np.int32))                                     # no such mask
    refused(ERR_INVALID, mask_id=np.array([-2, 0], np.int32))
    refused(ERR_INVALID, req=(np.array([1, 1, 1], np.uint32), np.array([7], np.uint32)))         # req_ptr does not start at 0
    refused(ERR_INVALID, exc=(np.array([0, 1, 0], np.uint32), np.array([7], np.uint32)))         # exc_ptr decreases
    refused(ERR_UNSUPPORTED, req=pack_pairs([list(range(17)), []]))                              # 17 distinct constraint terms
    refused(ERR_INVALID, ranges=engine.pack_doc_ranges([[(4, 0, 1)], []]))                       # a clause on a field that is not there
    refused(ERR_INVALID, ranges=(np.array([0, 1, 0], np.uint32), engine.pack_doc_ranges([[(0, 0, 1)]])[1]))
    refused(ERR_UNSUPPORTED, ranges=engine.pack_doc_ranges([[(0, 0, 1)] * 5, []]))               # five clauses
    refused(ERR_INVALID, m=0)
    refused(ERR_INVALID, first=-1)
    refused(ERR_UNSUPPORTED, first=MAX_TOPK - 3)                                                 # first + m = SS_MAX_TOPK + 1
    refused(ERR_UNSUPPORTED, first=2 ** 31 - 1)                                                  # ... computed without overflow
    # the raw ABI: NULL pointers and negative counts
    ptr = lambda a: a.ctypes.data                                                                 # noqa: E731
    args = lambda **o: [o.get("s", sc.h), o.get("n_q", 2), o.get("q_ptr", ptr(q_ptr)), o.get("q_terms", ptr(q_terms)), None, None, None, None, None,   # noqa: E731
                        None, None, o.get("first", 0), o.get("m", 4), o.get("groups", ptr(out[0])), o.get("n_out", ptr(out[1])),
                        ptr(out[2]), ptr(out[3]), ptr(out[4])]
    for code, o in ((ERR_INVALID, dict(s=None)), (ERR_INVALID, dict(n_q=-1)), (ERR_INVALID, dict(q_ptr=None)), (ERR_INVALID, dict(q_terms=None)),
                    (ERR_INVALID, dict(groups=None)), (ERR_INVALID, dict(n_out=None)), (ERR_INVALID, dict(m=-1)),
                    (ERR_UNSUPPORTED, dict(m=2 ** 31 - 1, first=2 ** 31 - 1)), (ERR_UNSUPPORTED, dict(m=MAX_TOPK + 1))):
        assert lib.ss_top_groups(*args(**o)) == code, o
        assert [a.tobytes() for a in out] == before
    for o in (dict(), dict(m=0), dict(first=-1), dict(m=MAX_TOPK, first=1), dict(q_ptr=None, groups=None, n_out=None)):
        assert lib.ss_top_groups(*args(n_q=0, **o)) == 0 and [a.tobytes() for a in out] == before    # n_q == 0 comes first: SS_OK, nothing done
    assert lib.ss_scorer_group_values(None, None, None) == ERR_INVALID
    sc.set_doc_groups(None)                                                                      # no group table
    refused(ERR_STATE)
    assert lib.ss_top_groups(*args(n_q=0)) == 0 and [a.tobytes() for a in out] == before


def test_too_many_query_terms(ss_ctx):
    """65 distinct usable terms in one query are refused as ss_facet_counts refuses them; 64 are counted"""
    n_docs, n_terms = 40, 70
    ptr = np.arange(n_terms + 1, dtype=np.uint64)
    doc = (np.arange(n_terms) % n_docs).astype(np.uint32)
    table = (ptr, doc, np.ones(n_terms, np.float32))
    sc, ti, bi = make_scorer(ss_ctx, n_docs, table, table, np.ones(n_docs), np.ones(n_docs))
    try:
        sc.set_doc_groups((np.arange(n_docs) % 7).astype(np.uint32))
        out = (filled((1, 4), GC), filled(1, np.int32), None, None, None)
        with pytest.raises(SpaghettiError) as ei:
            sc.top_groups(np.array([0, 65], np.uint32), np.arange(65, dtype=np.uint32), 0, 4, out=out)
        assert ei.value.code == ERR_UNSUPPORTED and out[0].tobytes() == bytes([FILL]) * 32 and out[1].tobytes() == bytes([FILL]) * 4
        rows, n_out, n_groups, n_ungrouped, n_match = sc.top_groups(np.array([0, 66], np.uint32),
                                                                    np.concatenate([np.arange(64), [0, UNKNOWN]]).astype(np.uint32), 0, 8)
        assert n_match.tolist() == [40] and n_groups.tolist() == [7] and n_out.tolist() == [7] and n_ungrouped.tolist() == [0]
        assert rows[0, :7].tolist() == [(g, 6) for g in range(5)] + [(5, 5), (6, 5)]
    finally:
        close_all(sc, ti, bi)
