"""ss_graph_create / ss_graph_apply_delta (csrc/graph.hip) on inputs built to reach the paths that no R-MAT graph reaches.

Nothing reads the layout back, so every check is on what the ABI hands out: PageRank against the oracle on the same CSR (equal
iteration counts, rtol 1e-12, eps 1e-10, K = 1 and K = 16 so that both sweep families read the layout), two builds of one graph
bit for bit, and every field of ss_graph_info against tests/graph_layout_model.py.  Each test asserts with the model, on its own
input and BEFORE it builds anything, that the input selects the path it is there for (tests/test_graph_layout_cpu.py makes the same
assertions without a GPU).

  path in graph.hip                                            test here                               model predicate
  -----------------------------------------------------------  --------------------------------------  ---------------------------------
  build(): second copy of the runs, n_runs > S                 test_readback_paths, S = 1, 8           more_runs_than(lay, c, S)
  build(): n_runs == S, k_pack_readback's min(r_n, spec)       test_readback_paths, S = 9              not more_runs_than(lay, c, 9) and
                                                                                                       more_runs_than(lay, c, 8)
  build(): n_runs < S (the only one other tests run)           test_readback_paths, S = 10, default    not more_runs_than(lay, c, S)
  chunk_rows() under k_permute_rows on a shard: bisection      test_chunk_corners_on_shards            chunk_on_bisection(lay.in_ptr)
    over the edge-less rows and the tail rows between the
    two id ranges
  ... a row that starts on a chunk boundary / over 3 chunks    test_chunk_corners_on_shards            row_on_chunk_boundary, row_spans_chunks
  k_delta_edges / k_delta_degrees: changed row over chunks     test_delta_seams[long_row]              row_spans_chunks(new out_ptr, 3)
  ... changed rows that begin and end on chunk boundaries      [rows_on_chunk_boundaries]              rows_on_chunk_boundary(new out_ptr)
  ... e_new a multiple of 2048, last row on the last slot      [last_row_ends_on_last_slot]            ptr[n] % 2048 == 0, ptr[n] > ptr[n - 1]
  ... > 8192 edge-less rows inside one chunk of the new CSR    [empty_stretch]                         chunk_on_bisection(new out_ptr)
  ... changed id >= n_old with children / growth alone         [new_page_with_children], [growth_only] (the delta itself)
  ... e = 0 before the delta, e_new = 0 after it, edges again  [from_and_to_zero_edges]                ptr[n] of every step
  ... `changed` not ascending                                  every delta of test_delta_seams         changed != sorted(changed)
  k_permute_rows: a parent twice in one in-list, self-loops    test_parallel_edges_and_self_loops      a (parent, child) key counted > 1
  ss_graph_create's refusals, every field of ss_graph_info     test_create_refusals, test_graph_info   -

Why S = 8, 9, 10 take the branches named, with 9 runs in each class on every rank (nine_runs_graph): build() clamps the option
"graph.readback_runs" to RLE_SPEC = S, k_pack_readback copies min(r_n[c], S) runs of class c into the block, and the host takes
`n_runs <= RLE_SPEC` from the block, anything else by the second copy from r_val / r_cnt.  S = 8: 9 <= 8 is false — second copy, and
the kernel's clamp min(9, 8) is the one that keeps it inside the block.  S = 9: 9 <= 9 — the block, filled to its last word.
S = 10: the block with a word to spare.  S = 1: the block is 80 bytes and both classes take the second copy."""
import ctypes as C

import numpy as np
import pytest

from spaghettisearch_amd import engine, synth
from tests import graph_layout_model as M
from tests import pr_graphs as G

pytestmark = pytest.mark.gpu
D, EPS = 0.75, 1e-10
KS = (1, 16)
_ref = {}


def reference(oracle, key, n, ptr, dst):
    """{K: (ranks, iterations)} of the oracle on this CSR, computed once per key"""
    if key not in _ref:
        _ref[key] = {k: oracle.pagerank(n, ptr, dst, D, EPS, synth.topic_sizes(n, k)) for k in KS}
    return _ref[key]


def assert_meets_oracle(got, ref):
    for k in KS:
        assert got[k][1].tolist() == ref[k][1].tolist(), k
        np.testing.assert_allclose(got[k][0], ref[k][0], rtol=1e-12)


def assert_same_bytes(a, b):
    for k in KS:
        assert a[k][1].tolist() == b[k][1].tolist() and a[k][0].tobytes() == b[k][0].tobytes(), k


def assert_info(g, n, ptr, dst):
    assert M.info_of(g.info()) == M.info(M.layout(n, ptr, dst, g.rank, g.world))


def run(ss_ctx, n, ptr, dst, world=1):
    """build the graph (all `world` shards of it), compare every shard's info with the model, -> {K: (ranks, iterations)}"""
    graphs = [engine.Graph(ss_ctx, n, ptr, dst, rank=r, world=world) for r in range(world)]
    try:
        for g in graphs:
            assert_info(g, n, ptr, dst)
        if world == 1:
            return {k: graphs[0].pagerank(D, EPS, synth.topic_sizes(n, k)) for k in KS}
        return {k: engine.Graph.pagerank_group(graphs, D, EPS, synth.topic_sizes(n, k)) for k in KS}
    finally:
        for g in graphs:
            g.close()


# ---- 1. the read-back of the in-degree runs -------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 3])
def test_readback_paths(ss_ctx, oracle, world):
    n, ptr, dst = G.nine_runs_graph()
    lays = [M.layout(n, ptr, dst, r, world) for r in range(world)]
    assert all(len(lay.runs[c][0]) == 9 for lay in lays for c in (0, 1))
    ref = reference(oracle, "nine_runs", n, ptr, dst)
    default = run(ss_ctx, n, ptr, dst, world)
    assert_meets_oracle(default, ref)
    for opts, over in (({"graph__readback_runs": 1}, True), ({"graph__readback_runs": 8}, True), ({"graph__readback_runs": 9}, False),
                       ({"graph__readback_runs": 10}, False), ({"graph__readback_runs": 1, "graph__late_free": 0}, True)):
        s = opts["graph__readback_runs"]
        assert all(M.more_runs_than(lay, c, s) is over for lay in lays for c in (0, 1)), s      # the side of S every rank's classes fall on
        assert not any(M.more_runs_than(lay, c, M.READBACK_RUNS) for lay in lays for c in (0, 1))
        with ss_ctx.options(**opts):
            got = run(ss_ctx, n, ptr, dst, world)
        assert_same_bytes(got, default)
        assert_meets_oracle(got, ref)


def test_readback_runs_is_clamped(ss_ctx, oracle):
    # 0 and a value above the largest block are taken as 1 and 8192
    n, ptr, dst = G.nine_runs_graph()
    default = run(ss_ctx, n, ptr, dst)
    for v in (0, -5, 1 << 20):
        with ss_ctx.options(graph__readback_runs=v):
            assert_same_bytes(run(ss_ctx, n, ptr, dst), default)


# ---- 2. chunk corners on shards -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3, 4])
def test_chunk_corners_on_shards(ss_ctx, oracle, world):
    n, ptr, dst = G.chunk_corner_graph(G.CORNER_LINKERS[world])
    # the out-edge direction (k_edge_parents: dangling sources in id order), the same on every rank
    assert M.chunk_on_bisection(ptr) and M.row_on_chunk_boundary(ptr) and M.row_spans_chunks(ptr, 3)
    # the in-edge direction (k_permute_rows: the pages nobody links to at the end of the non-dangling class, then the tail rows)
    in_ptrs = [M.layout(n, ptr, dst, r, world).in_ptr for r in range(world)]
    assert any(M.chunk_on_bisection(p) for p in in_ptrs)
    assert any(M.row_on_chunk_boundary(p) for p in in_ptrs)
    assert any(M.row_spans_chunks(p, 3) for p in in_ptrs)
    got = run(ss_ctx, n, ptr, dst, world)                       # (compares every rank's ss_graph_info with the model)
    assert_meets_oracle(got, reference(oracle, ("corner", G.CORNER_LINKERS[world]), n, ptr, dst))


# ---- 3. delta seams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("late_free", [1, 0])
@pytest.mark.parametrize("seam", G.DELTA_SEAM_NAMES)
def test_delta_seams(ss_ctx, oracle, seam, late_free):
    rows, steps = G.delta_seams()[seam]
    ptr, dst = G.csr_of(rows)
    with ss_ctx.options(graph__late_free=late_free):
        g = engine.Graph(ss_ctx, len(rows), ptr, dst)
        try:
            for i, (n_new, changed, lists) in enumerate(steps):
                assert len(changed) < 2 or [int(v) for v in changed] != sorted(int(v) for v in changed)
                nptr, nchildren = G.csr_of(lists)
                g.apply_delta(n_new, np.array(changed, dtype=np.uint32), nptr, nchildren)
                rows = G.apply_rows(rows, n_new, changed, lists)
                ptr2, dst2 = G.csr_of(rows)
                assert_info(g, n_new, ptr2, dst2)
                got = {k: g.pagerank(D, EPS, synth.topic_sizes(n_new, k)) for k in KS}
                fresh = run(ss_ctx, n_new, ptr2, dst2)
                assert_same_bytes(got, fresh)
                ref = reference(oracle, (seam, i), n_new, ptr2, dst2)
                assert_meets_oracle(got, ref)
                assert_meets_oracle(fresh, ref)
        finally:
            g.close()


# ---- 4. parallel edges and self-loops -------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2])
def test_parallel_edges_and_self_loops(ss_ctx, oracle, world):
    n, ptr, dst = G.multi_edge_graph()
    src = np.repeat(np.arange(n), np.diff(ptr.astype(np.int64)))
    key, count = np.unique(src * n + dst.astype(np.int64), return_counts=True)
    assert count.max() == 5 and np.any(key // n == key % n)         # a parent five times in one in-list; self-loops
    got = run(ss_ctx, n, ptr, dst, world)
    assert_meets_oracle(got, reference(oracle, "multi_edge", n, ptr, dst))


# ---- 5. refusals and info -------------------------------------------------------------------------------------------------
def test_create_refusals(ss_ctx, oracle):
    u64, u32 = (lambda *v: np.array(v, dtype=np.uint64)), (lambda *v: np.array(v, dtype=np.uint32))
    ptr, dst = u64(0, 1, 2), u32(1, 0)
    cases = {"out_ptr[0] != 0": (2, 2, u64(1, 1, 2), dst, 0, 1),
             "out_ptr[n] != n_edges": (2, 2, u64(0, 1, 1), dst, 0, 1),
             "n_nodes = 0": (0, 0, u64(0), None, 0, 1),
             "rank < 0": (2, 2, ptr, dst, -1, 1),
             "rank >= world": (2, 2, ptr, dst, 2, 2),
             "world < 1": (2, 2, ptr, dst, 0, 0),
             "NULL out_dst with edges": (2, 2, ptr, None, 0, 1)}
    create = ss_ctx.lib.ss_graph_create
    for name, (n, e, p, d, rank, world) in cases.items():
        out = C.c_void_p(0xDEAD0)
        rc = create(ss_ctx.h, n, e, p.ctypes.data, None if d is None else d.ctypes.data, rank, world, C.byref(out))
        assert rc == 1, name                                         # SS_ERR_INVALID
        assert out.value is None, name                               # *out is NULL
    assert create(ss_ctx.h, 2, 2, ptr.ctypes.data, dst.ctypes.data, 0, 1, None) == 1, "NULL out"
    # the context still builds a good graph
    n, e = 3000, 14000
    ptr, dst = synth.rmat_graph(n, e, seed=8)
    assert_meets_oracle(run(ss_ctx, n, ptr, dst), reference(oracle, "after_refusals", n, ptr, dst))


@pytest.mark.parametrize("world", [1, 4])
@pytest.mark.parametrize("graph", ["corner", "rmat"])
def test_graph_info(ss_ctx, graph, world):
    n, ptr, dst = G.chunk_corner_graph(G.CORNER_LINKERS[world]) if graph == "corner" else (20000,) + synth.rmat_graph(20000, 100000, seed=12)
    for r in range(world):
        g = engine.Graph(ss_ctx, n, ptr, dst, rank=r, world=world)
        try:
            lay = M.layout(n, ptr, dst, r, world)
            gi = g.info()
            assert (gi.n_nodes, gi.n_edges, gi.n_nondangling) == (n, len(dst), lay.n_nd)
            assert (gi.n_rows_local, gi.n_edges_local, gi.max_indeg) == (lay.cnt_nd + lay.cnt_d, lay.e_local, lay.max_indeg)
            assert (gi.rank, gi.world) == (r, world)
            assert M.info_of(gi) == M.info(lay)
        finally:
            g.close()
