"""class_boundary_graph() (tests/pr_graphs.py) reaches what it claims, proved without a GPU: its two in-degree tables go through the
planner (tests/pr_plan_harness.cpp) with each parameter set the library picks for a small graph (plan_options and pick_kernel in
csrc/pagerank.hip), and the items that come out must hold every row class of that kernel for non-dangling AND dangling rows, hubs
with a one-edge and with a full last piece, ticket indices above 0, exact-degree runs of several items with a short last one, every
chunks-per-row count below T_QUAD, and several items of edge-less rows.  The same holds for every shard of world 2 and 3 (the deal of
tests/graph_layout_model.py: sorted position i of a class goes to rank i % W).  A second test shows that the CPU oracle itself tells
a boundary row from the same row without its last in-edge by far more than the tolerance tests/test_gpu_pr_classes.py compares at.
These are conditions on the graph, not measurements; each test prints one line of item counts per parameter set."""
from collections import Counter

import numpy as np
import pytest

from tests import pr_graphs
from tests.test_pr_plan_cpu import (CH, SEGW, T_DEG, T_MULTI, V_DEG, V_QUAD, V_ROWW, V_SEG, V_ZERO, W_GROUP, W_SEG, W_WAVE, W_ZERO,
                                    check_cut, check_placement, harness, plan)  # noqa: F401  (harness: the module's fixture)

KIND_NAMES = {W_SEG: "W_SEG", W_WAVE: "W_WAVE", W_GROUP: "W_GROUP", W_ZERO: "W_ZERO", V_SEG: "V_SEG", V_ROWW: "V_ROWW", V_QUAD: "V_QUAD",
              V_DEG: "V_DEG", V_ZERO: "V_ZERO"}
# name -> (gw the items are cut for, lane_rows, t_quad, item_turns, deal_global): what ss_pr_create uses at up to 4M rows
#   k_pr_sweep<8> (K = 3 .. 8), k_pr_sweep<16> (K = 9 .. 16): T_QUAD 128, 4 turns per V_DEG item
#   k_pr_sweep_n<1|2> (K = 1, 2): items cut for 8-lane groups with a lane per short row, T_QUAD 256, 1 turn (K = 1 deals from one global order)
#   k_pr_step<1|2> ("pr.force_narrow"): block items
PARAMETER_SETS = {"k_pr_sweep<8>": (8, 0, 128, 4, 2), "k_pr_sweep<16>": (16, 0, 128, 4, 2), "k_pr_sweep_n": (8, 1, 256, 1, 1),
                  "k_pr_step<1>": (1, 0, 128, 4, 2), "k_pr_step<2>": (2, 0, 128, 4, 2)}
WAVE_SETS = [name for name, p in PARAMETER_SETS.items() if p[0] >= 8]


@pytest.fixture(scope="module")
def tables():
    n, ptr, dst = pr_graphs.class_boundary_graph()
    nd, d, rows_nd, rows_d = pr_graphs.class_degree_tables(n, ptr, dst)
    return nd, d, rows_nd, rows_d


def run_plan(exe, nd, d, name, nblocks=3):
    gw, lane, t_quad, turns, deal_global = PARAMETER_SETS[name]
    r = plan(exe, nd, d, gw, lane, nblocks, t_quad, turns, -1, deal_global)
    check_cut(r, nd, d, gw, lane, t_quad)
    if gw >= 8:
        check_placement(r, nblocks)
    return r


def counts_line(tag, r, sl_nd):
    c = Counter((kind, row >= sl_nd) for kind, row, *_ in r["item"])
    return f"class graph items, {tag}: " + "  ".join(f"{KIND_NAMES[k]} {c[(k, False)]} non-dangling / {c[(k, True)]} dangling"
                                                     for k in sorted({k for k, _ in c}))


def assert_reach(r, nd, d, name, whole_graph):
    """every claim of the module's docstring for one plan; whole_graph: the hubs named in the issue are all in these tables"""
    gw, lane, t_quad, turns, _ = PARAMETER_SETS[name]
    sl_nd = len(nd)
    deg = lambda row: nd[row] if row < sl_nd else d[row - sl_nd]
    for cls, (lo, hi) in {"non-dangling": (0, sl_nd), "dangling": (sl_nd, sl_nd + len(d))}.items():
        items = [it for it in r["item"] if lo <= it[1] < hi]
        kinds = Counter(it[0] for it in items)
        zero_kind = V_ZERO if gw >= 8 else W_ZERO
        # every item kind of the kernel (edge-less rows are work only where they have children)
        want = ({V_SEG, V_ROWW, V_QUAD, V_DEG} if gw >= 8 else {W_SEG, W_WAVE, W_GROUP}) | ({zero_kind} if cls == "non-dangling" else set())
        assert set(kinds) == want, (name, cls, kinds)
        if cls == "non-dangling":
            assert kinds[zero_kind] >= 2
        # hubs: at least two tickets, and pieces whose lengths follow from the degree
        seg_kind, seg_w = (V_SEG, SEGW) if gw >= 8 else (W_SEG, 128 * (64 // gw))
        pieces = {}
        for kind, row, sg, ns, sbase, tix in items:
            if kind == seg_kind:
                pieces.setdefault(row, []).append(min(seg_w, deg(row) - sg * seg_w))
        assert len({it[5] for it in items if it[0] == seg_kind and it[3] > 1}) >= 2, (name, cls)
        assert all(sum(p) == deg(row) and min(p) >= 1 for row, p in pieces.items())
        if not whole_graph:
            continue                                                   # a shard: the kinds and the tickets are what is asked of it
        last = {deg(row): p[-1] for row, p in pieces.items()}
        nslot = 64 // gw
        in_kind = lambda k: {deg(q) for kind, row, count, *_ in items if kind == k for q in range(row, row + count)}
        if gw < 8:
            # a one-edge last piece, one full piece, and k_pr_step's thresholds inside the classes they separate
            assert last[3 * seg_w + 1] == 1 and last[seg_w] == seg_w and last[seg_w + 1] == 1
            assert {2 * nslot - 1, 2 * nslot} <= in_kind(W_GROUP) and {2 * nslot + 1, 32 * nslot - 1, 32 * nslot} <= in_kind(W_WAVE)
            assert 32 * nslot + 1 in last
            continue
        assert last[3 * SEGW + 1] == 1 and last[3 * SEGW] == SEGW and last[2 * SEGW + 1] == 1 and len(pieces) >= 8
        # exact-degree runs: every degree 1 .. 8, at least three items, all full but the last
        for D in range(1, T_DEG + 1):
            run = [it[2] for it in items if it[0] == V_DEG and it[3] == D]
            per_item = 64 * turns if lane else nslot * (8 if D <= 2 else 4 if D <= 4 else 2) * turns
            assert len(run) >= 3 and set(run[:-1]) == {per_item} and 0 < run[-1] < per_item, (name, cls, D, run)
        # a V_QUAD item for the chunks-per-row count of every threshold degree up to T_QUAD; at one and two chunks more rows than an
        # item holds, the last item not filling the lane groups
        quad = [(it[2], it[3]) for it in items if it[0] == V_QUAD]
        want_nch = {-(-v // CH) for v in pr_graphs.CLASS_WAVE_DEGREES + pr_graphs.CLASS_STEP_DEGREES if T_DEG < v <= t_quad}
        assert want_nch <= {nch for _, nch in quad}, (name, cls)
        for nch in (1, 2):
            rows = [count for count, c in quad if c == nch]
            max_groups = min(gw, max(1, 2 * turns // nch))
            assert sum(rows) > max_groups * nslot and sum(rows) % 4 != 0 and rows[-1] % nslot != 0, (name, cls, nch, rows)
            assert set(rows[:-1]) == {max_groups * nslot}
        # both sides of T_QUAD and of T_MULTI
        assert {t_quad + 1, T_MULTI} <= {deg(it[1]) for it in items if it[0] == V_ROWW}
        assert t_quad in in_kind(V_QUAD) and T_MULTI + 1 in last


def test_graph_holds_the_multiset_in_both_classes(tables):
    nd, d, rows_nd, rows_d = tables
    want = pr_graphs.class_degree_multiset()
    assert [x for x in nd if x > 0] == want and [x for x in d if x > 0] == want
    assert nd.count(0) == pr_graphs.CLASS_ZERO_ND >= 2 * 128 + 1 and d.count(0) == pr_graphs.CLASS_ZERO_D > 0
    n, ptr, dst = pr_graphs.class_boundary_graph()
    assert 29000 <= n <= 31000
    outdeg = np.diff(ptr.astype(np.int64))
    src = np.repeat(np.arange(n), outdeg)
    assert len(np.unique(src * n + dst.astype(np.int64))) == len(dst)                   # unique edges
    assert len(np.unique(outdeg[rows_nd[np.array(nd) == 0]])) > 64                      # shared rows span more than a wave
    assert rows_nd.max() - rows_nd.min() + 1 > len(rows_nd) and rows_d.max() - rows_d.min() + 1 > len(rows_d)   # no class is a range of ids


@pytest.mark.parametrize("name", list(PARAMETER_SETS))
def test_every_row_class_is_reached_in_both_classes(harness, tables, name):  # noqa: F811
    nd, d, _, _ = tables
    r = run_plan(harness, nd, d, name)
    print(counts_line(name, r, len(nd)))
    assert_reach(r, nd, d, name, whole_graph=True)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", WAVE_SETS)
def test_every_shard_owns_every_wave_item_class(harness, tables, name, world):  # noqa: F811
    # the sharded GPU cases run the wave-item kernels: each rank gets hub pieces and items of every other class, for both row classes
    nd, d, _, _ = tables
    for rank in range(world):
        nd_r, d_r = nd[rank::world], d[rank::world]
        r = run_plan(harness, nd_r, d_r, name)
        print(counts_line(f"{name} rank {rank} of {world}", r, len(nd_r)))
        assert_reach(r, nd_r, d_r, name, whole_graph=False)


SENSITIVE_DEGREES = [3 * SEGW + 1, T_MULTI + 1, T_MULTI, 257, 129, 17, 9, 8, 1]


def without_last_in_edge(n, ptr, dst, v):
    """the CSR without the in-edge of v that comes last in its row of the in-edge lists (the largest parent id)"""
    ptr = ptr.astype(np.int64)
    src = np.repeat(np.arange(n), np.diff(ptr))
    at = np.flatnonzero(dst == v)
    cut = at[np.argmax(src[at])]
    ptr2 = ptr.copy()
    ptr2[src[cut] + 1:] -= 1
    return ptr2.astype(np.uint64), np.delete(dst, cut)


def test_oracle_tells_a_row_from_the_row_without_its_last_edge(oracle, tables):
    """After 2 sweeps the rank of a boundary row differs by at least 1e-9 relative from that of the same row with one in-edge fewer:
    three orders of magnitude above the 1e-12 the GPU tests compare at — a kernel that drops such an edge cannot pass them."""
    nd, d, rows_nd, rows_d = tables
    n, ptr, dst = pr_graphs.class_boundary_graph()
    n_topic = pr_graphs.topic_sizes(n, 2)
    ref, _ = oracle.pagerank(n, ptr, dst, 0.75, -1.0, n_topic, max_iter=2)
    for degs, rows in ((nd, rows_nd), (d, rows_d)):
        for deg in SENSITIVE_DEGREES:
            v = int(rows[degs.index(deg)])
            ptr2, dst2 = without_last_in_edge(n, ptr, dst, v)
            assert len(dst2) == len(dst) - 1 and np.count_nonzero(dst2 == v) == deg - 1
            got, _ = oracle.pagerank(n, ptr2, dst2, 0.75, -1.0, n_topic, max_iter=2)
            rel = np.abs(got[:, v] - ref[:, v]) / np.abs(ref[:, v])
            assert rel.min() >= 1e-9, (deg, rel)
