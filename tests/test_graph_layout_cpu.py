"""tests/graph_layout_model.py against hand-worked values, and the graph builders of tests/pr_graphs.py against the predicates that
tests/test_gpu_graph_paths.py relies on (no GPU: the same assertions run there again in front of every build)."""
import numpy as np
import pytest

from tests import graph_layout_model as M
from tests import pr_graphs as G

# ten nodes, worked by hand.  children: 0 -> 1 2 3, 1 -> 2 3, 2 -> 3, 4 -> 3 9, 5 -> 2, 7 -> 9; 3, 6, 8, 9 are dangling
HAND_ROWS = [[1, 2, 3], [2, 3], [3], [], [3, 9], [2], [], [9], [], []]


def hand_graph():
    ptr, dst = G.csr_of([np.array(r, dtype=np.uint32) for r in HAND_ROWS])
    return 10, ptr, dst


def runs_as_lists(lay):
    return [[v.tolist(), l.tolist()] for v, l in lay.runs]


def test_hand_graph_world_1():
    lay = M.layout(*hand_graph())
    assert lay.outdeg.tolist() == [3, 2, 1, 0, 2, 1, 0, 1, 0, 0]
    assert lay.indeg.tolist() == [0, 1, 3, 4, 0, 0, 0, 0, 0, 2]
    assert lay.cls.tolist() == [0, 0, 0, 1, 0, 0, 1, 0, 1, 1]
    assert lay.order.tolist() == [2, 1, 0, 4, 5, 7, 3, 9, 6, 8]          # class, in-degree descending, id ascending
    assert (lay.n_nd, lay.n_d, lay.sl_nd, lay.sl_d, lay.cnt_nd, lay.cnt_d) == (6, 4, 6, 4, 6, 4)
    assert lay.in_ptr.tolist() == [0, 3, 4, 4, 4, 4, 4, 8, 10, 10, 10]
    assert runs_as_lists(lay) == [[[3, 1, 0], [1, 1, 4]], [[4, 2, 0], [1, 1, 2]]]
    assert M.info(lay) == dict(n_nodes=10, n_edges=10, n_nondangling=6, n_rows_local=10, n_edges_local=10, max_indeg=4, rank=0, world=1)
    assert M.more_runs_than(lay, 0, 2) and not M.more_runs_than(lay, 0, 3) and M.more_runs_than(lay, 1, 1)


def test_hand_graph_world_3():
    n, ptr, dst = hand_graph()
    lays = [M.layout(n, ptr, dst, r, 3) for r in range(3)]
    tail = 2 + M.TAIL_SUM_ROWS
    for lay in lays:
        assert (lay.sl_nd, lay.sl_d) == (2 + tail, 2) and len(lay.in_ptr) == 2 + tail + 2 + 1
    assert [lay.rows_nd.tolist() for lay in lays] == [[2, 4], [1, 5], [0, 7]]          # sorted position i -> rank i % 3, place i // 3
    assert [lay.rows_d.tolist() for lay in lays] == [[3, 8], [9], [6]]
    assert [(lay.cnt_nd, lay.cnt_d) for lay in lays] == [(2, 2), (2, 1), (2, 1)]
    assert lays[0].in_ptr.tolist() == [0] + [3] * (1 + tail + 1) + [7, 7]               # the tail rows sit between the two classes
    assert lays[1].in_ptr.tolist() == [0] + [1] * (1 + tail + 1) + [3, 3]
    assert lays[2].in_ptr.tolist() == [0] * (2 + tail + 2 + 1)
    assert [runs_as_lists(lay) for lay in lays] == [[[[3, 0], [1, 1]], [[4, 0], [1, 1]]], [[[1, 0], [1, 1]], [[2], [1]]], [[[0], [2]], [[0], [1]]]]
    assert [M.info(lay)["n_edges_local"] for lay in lays] == [7, 3, 0]
    assert [M.info(lay)["max_indeg"] for lay in lays] == [4, 2, 0]
    assert [M.info(lay)["n_rows_local"] for lay in lays] == [4, 3, 3]


def test_chunk_first_rows_by_hand():
    C = M.EK_CHUNK
    ptr = [0, C, C, 5000, 5000, 3 * C]                  # row 1 is empty, row 2 starts on a chunk boundary and runs into the third chunk
    r_lo, r_hi = M.chunk_first_rows(ptr)
    assert r_lo.tolist() == [0, 2, 2] and r_hi.tolist() == [2, 2, 4]
    assert M.rows_on_chunk_boundary(ptr).tolist() == [2]
    assert M.row_spans_chunks(ptr, 2) and not M.row_spans_chunks(ptr, 3) and not M.chunk_on_bisection(ptr)
    assert M.row_spans_chunks([0, 1, 2 * C + 1], 3) and not M.row_spans_chunks([0, 1, 2 * C], 3)      # slots 1 .. 2 C: three chunks
    # 8193 rows between the holders of two neighbouring chunk starts: over the limit by one; 8192: not yet
    for rows, want in ((M.BISECT_ROWS + 1, True), (M.BISECT_ROWS, False)):
        ptr = np.concatenate(([0], np.full(rows, 5), [2 * C + 7]))                      # row 0 holds slot 0, row `rows` slots 2048 and 4096
        r_lo, r_hi = M.chunk_first_rows(ptr)
        assert r_lo.tolist() == [0, rows, rows] and r_hi.tolist() == [rows, rows, rows]
        assert M.chunk_on_bisection(ptr) is want
    assert M.chunk_first_rows([0, 0, 0])[0].tolist() == []


def test_csr_from_edges_keeps_parallel_edges():
    ptr, dst = M.csr_from_edges(4, [2, 0, 2, 2, 0], [1, 3, 1, 0, 3])
    assert ptr.tolist() == [0, 2, 2, 5, 5] and dst.tolist() == [3, 3, 0, 1, 1]


# ---- the builders meet what the GPU tests say of them ---------------------------------------------------------------------
def test_nine_runs_graph_has_nine_runs_per_class_on_every_rank():
    n, ptr, dst = G.nine_runs_graph()
    assert n <= 150000 and len(dst) <= 300000
    for world in (1, 3):
        for r in range(world):
            lay = M.layout(n, ptr, dst, r, world)
            for c in (0, 1):
                assert len(lay.runs[c][0]) == 9
                # which side of S = 1, 8, 9, 10, 8192 the class falls on: over, over, NOT over (equal), not over, not over
                assert [M.more_runs_than(lay, c, s) for s in (1, 8, 9, 10, M.READBACK_RUNS)] == [True, True, False, False, False]


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_chunk_corner_graph_reaches_the_corners_on_shards(world):
    n, ptr, dst = G.chunk_corner_graph(G.CORNER_LINKERS[world])
    assert n <= 150000 and len(dst) <= 300000 and len(dst) % M.EK_CHUNK == 0 and int(ptr[n]) == len(dst) > int(ptr[n - 1])
    # the out-edge CSR (k_edge_parents), the same on every rank
    assert M.chunk_on_bisection(ptr) and M.row_on_chunk_boundary(ptr) and M.row_spans_chunks(ptr, 3)
    # the local in_ptr (k_permute_rows): here EVERY rank has all three
    for r in range(world):
        lay = M.layout(n, ptr, dst, r, world)
        assert M.chunk_on_bisection(lay.in_ptr) and M.row_on_chunk_boundary(lay.in_ptr) and M.row_spans_chunks(lay.in_ptr, 3), (world, r)
        # ... and the bisected chunk is the one that holds the edge-less end of the non-dangling class and the tail rows
        r_lo, r_hi = M.chunk_first_rows(lay.in_ptr)
        c = int(np.argmax(r_hi - r_lo))
        assert r_lo[c] < lay.cnt_nd <= lay.sl_nd <= r_hi[c]


def test_multi_edge_graph_has_what_it_says():
    n, ptr, dst = G.multi_edge_graph()
    src = np.repeat(np.arange(n), np.diff(ptr.astype(np.int64)))
    key, count = np.unique(src * n + dst.astype(np.int64), return_counts=True)
    assert 1900 <= n <= 2100
    assert set(count.tolist()) == {1, 2, 3, 4, 5} and 0.08 < (count[count > 1].sum() - 5) / len(dst) and (count > 1).sum() >= 0.09 * len(key)
    loops = key[key // n == key % n]
    assert 0.008 * len(dst) <= len(loops) <= 0.012 * len(dst)
    assert dst[int(ptr[n - 2]):int(ptr[n - 1])].tolist() == [n - 2] and dst[int(ptr[n - 1]):].tolist() == [7] * 5
    # a parent that repeats inside one in-list: the same (parent, child) key more than once
    assert np.any(count > 1)


def test_delta_seams_are_where_they_claim():
    seams = G.delta_seams()
    assert tuple(seams) == G.DELTA_SEAM_NAMES
    C = M.EK_CHUNK
    after = {}
    for name, (base, steps) in seams.items():
        rows, out = base, []
        for n_new, changed, lists in steps:
            changed = [int(v) for v in changed]
            assert len(changed) < 2 or changed != sorted(changed), name                     # `changed` is not ascending
            assert len(set(changed)) == len(changed) and len(changed) == len(lists)
            assert all(len(np.unique(l)) == len(l) and (len(l) == 0 or int(max(l)) < n_new) for l in lists), name   # unique children, in range
            assert n_new >= len(rows) and n_new <= 150000
            out.append((len(rows), changed, G.csr_of(G.apply_rows(rows, n_new, changed, lists))[0].astype(np.int64)))
            rows = G.apply_rows(rows, n_new, changed, lists)
            assert int(out[-1][2][-1]) <= 300000
        after[name] = out
    n_old, changed, ptr = after["long_row"][0]
    assert ptr[12346] - ptr[12345] == 5000 and M.row_spans_chunks(ptr, 3)
    n_old, changed, ptr = after["rows_on_chunk_boundaries"][0]
    assert [int(ptr[v + 1] - ptr[v]) for v in (20000, 20001, 20002)] == [C] * 3 and ptr[20000] % C == 0 and ptr[20000] > 0
    assert set((20000, 20001, 20002)) <= set(M.rows_on_chunk_boundary(ptr).tolist())
    n_old, changed, ptr = after["last_row_ends_on_last_slot"][0]
    assert ptr[-1] % C == 0 and ptr[-1] > ptr[-2]
    n_old, changed, ptr = after["empty_stretch"][0]
    assert np.all(np.diff(ptr)[10000:19001] == 0) and ptr[19002] > ptr[19001] and ptr[10000] > 0 and M.chunk_on_bisection(ptr)
    n_old, changed, ptr = after["new_page_with_children"][0]
    assert len(ptr) - 1 > n_old and any(v >= n_old and ptr[v + 1] > ptr[v] for v in changed)
    n_old, changed, ptr = after["growth_only"][0]
    assert changed == [] and len(ptr) - 1 == n_old + 700
    (n0, _, p1), (_, _, p2), (_, _, p3) = after["from_and_to_zero_edges"]
    assert all(len(r) == 0 for r in seams["from_and_to_zero_edges"][0]) and p1[-1] > 0 and p2[-1] == 0 and p3[-1] > 0
