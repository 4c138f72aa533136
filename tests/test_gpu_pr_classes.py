"""The PageRank sweep kernels on class_boundary_graph() (tests/pr_graphs.py): rows on both sides of every planner threshold, as
non-dangling AND as dangling rows, hubs of several pieces in both classes, exact-degree runs and edge-less stretches of several
items with ragged tails.  tests/test_pr_class_graph_cpu.py proves on the CPU that the graph reaches every item kind of every kernel;
here every kernel instantiation runs it — k_pr_sweep<8|16>, k_pr_sweep_n<1|2>, k_pr_step<1|2> — alone, with the shared table rows
on and off, with the sweeps inside one launch, in the two-vector form, on shards, and under the planner options that only move
work.  Every comparison is against the CPU oracle with the gates of tests/test_gpu_pagerank.py: ranks at rtol 1e-12, equal
iteration counts, and bit equality where that module and tests/test_gpu_pr_shared_rows.py assert it.  Fixed-sweep runs of 1, 2 and
5 sweeps stand beside the runs to convergence: a wrong row class shows at the sweep where it happens."""
import numpy as np
import pytest

from spaghettisearch_amd import engine
from tests.pr_graphs import NARROW_VARIANTS, class_boundary_graph, topic_sizes
from tests.test_gpu_pr_shared_rows import assert_same, run_state

pytestmark = pytest.mark.gpu
D = 0.75
EPS = 1e-10
# (eps, max_iter): 1, 2 and 5 sweeps whatever the change, and to convergence.  The reference's normaliser makes every topic of this
# graph stop after 4 sweeps at 1e-10; at 1e-11 the topics with the larger sets stop after 4 and the others after 5 (the oracle's own
# L1 changes at sweep 4 run from 5e-13 to 5e-11 over the sixteen topic sizes), so the frozen-topic path runs beside live topics
MODES = [(-1.0, 1), (-1.0, 2), (-1.0, 5), (EPS, 0), (1e-11, 0)]

_ref = {}


def reference(oracle, k_topics, eps, max_iter):
    """the oracle's (ranks, iteration counts) on the class graph, computed once per (K, mode)"""
    key = (k_topics, eps, max_iter)
    if key not in _ref:
        n, ptr, dst = class_boundary_graph()
        rank, iters = oracle.pagerank(n, ptr, dst, D, eps, topic_sizes(n, k_topics), max_iter=max_iter)
        rank.setflags(write=False)
        iters.setflags(write=False)
        _ref[key] = rank, iters
    return _ref[key]


@pytest.fixture(scope="module")
def graph(ss_ctx):
    n, ptr, dst = class_boundary_graph()
    g = engine.Graph(ss_ctx, n, ptr, dst)
    yield g
    g.close()


def assert_meets_oracle(oracle, got, k_topics, eps, max_iter, note=None):
    rank, iters = got
    ref, ref_iters = reference(oracle, k_topics, eps, max_iter)
    assert iters.tolist() == ref_iters.tolist(), (note, eps, max_iter)
    if max_iter:
        assert iters.tolist() == [max_iter] * k_topics
    np.testing.assert_allclose(rank, ref, rtol=1e-12, err_msg=str((note, eps, max_iter)))


# K = 16, 9: k_pr_sweep<16>; K = 8, 5, 3: k_pr_sweep<8>
@pytest.mark.parametrize("k_topics", [16, 9, 8, 5, 3])
def test_wide_sweep_matches_the_oracle(ss_ctx, oracle, graph, k_topics):
    n_topic = topic_sizes(graph.n, k_topics)
    for eps, max_iter in MODES:
        assert_meets_oracle(oracle, graph.pagerank(D, eps, n_topic, max_iter=max_iter), k_topics, eps, max_iter)


# K = 1, 2: k_pr_sweep_n<K> (default), k_pr_sweep<8> padded, k_pr_step<K>
@pytest.mark.parametrize("k_topics", [1, 2])
def test_narrow_kernels_match_the_oracle_and_each_other(ss_ctx, oracle, graph, k_topics):
    n_topic = topic_sizes(graph.n, k_topics)
    for eps, max_iter in MODES:
        got = {}
        for variant, opts in NARROW_VARIANTS.items():
            with ss_ctx.options(**opts):
                got[variant] = graph.pagerank(D, eps, n_topic, max_iter=max_iter)
            assert_meets_oracle(oracle, got[variant], k_topics, eps, max_iter, variant)
        for variant in ("padded_8_wide", "block_items"):
            assert got[variant][1].tolist() == got["wave_items"][1].tolist()
            np.testing.assert_allclose(got[variant][0], got["wave_items"][0], rtol=1e-13, err_msg=variant)


@pytest.mark.parametrize("k_topics", [3, 16])
def test_shared_rows_on_and_off_are_bit_identical(ss_ctx, oracle, graph, k_topics):
    """"pr.share_zero_rows" 1 against 0: the 20800 rows without in-edges have 126 distinct out-degrees (two waves of shared rows); their
    gatherers are rows of every class, dangling ones too"""
    n_topic = topic_sizes(graph.n, k_topics)
    for eps, max_iter in MODES:
        sweeps = max_iter or None
        on = run_state(ss_ctx, graph, n_topic, 1, eps, 0, sweeps=sweeps)
        off = run_state(ss_ctx, graph, n_topic, 0, eps, 0, sweeps=sweeps)
        assert_same(on, off)                                           # ranks, read_local, iterations, total and delta: bit for bit
        assert_meets_oracle(oracle, (on[0], on[2]["iters"]), k_topics, eps, max_iter)
        assert np.array_equal(on[0], on[1])                            # read() == read_local() scattered by id: edge-less dangling rows too


@pytest.mark.parametrize("k_topics", [1, 2])
def test_sweeps_inside_one_launch_are_bit_identical(ss_ctx, oracle, graph, k_topics):
    """"pr.persistent" 0 | 1 | 2: the hubs' tickets (eight per class) are reused sweep after sweep inside one launch"""
    n_topic = topic_sizes(graph.n, k_topics)
    for eps, max_iter in ((EPS, 0), (-1.0, 5)):
        got = {}
        for mode in (0, 1, 2):                    # one launch per sweep; write-through hand-offs; release / acquire fences
            with ss_ctx.options(pr__persistent=mode):
                got[mode] = graph.pagerank(D, eps, n_topic, max_iter=max_iter)
        for mode in (1, 2):
            assert got[0][1].tolist() == got[mode][1].tolist(), (mode, eps)
            assert got[0][0].tobytes() == got[mode][0].tobytes(), (mode, eps)
        assert_meets_oracle(oracle, got[1], k_topics, eps, max_iter)
    # 3 + 1 + 5 sweeps inside launches == nine launches of one sweep
    xs = {}
    for mode, steps in ((0, (1,) * 9), (0, (3, 1, 5)), (1, (3, 1, 5)), (2, (3, 1, 5))):
        with ss_ctx.options(pr__persistent=mode):
            st = engine.PageRankState(graph, D, -1.0, n_topic, max_iter=0)
        try:
            st.begin()
            for m in steps:
                st.step(m)
            s = st.status()
            assert s["sweeps"] == 9 and s["iters"].tolist() == [9] * k_topics
            xs[mode, steps] = st.read()
        finally:
            st.close()
    singles = xs[0, (1,) * 9]
    assert all(x.tobytes() == singles.tobytes() for x in xs.values())
    np.testing.assert_allclose(singles, reference(oracle, k_topics, -1.0, 9)[0], rtol=1e-12)


@pytest.mark.parametrize("k_topics", [1, 3, 16])
def test_two_vector_form_matches_the_oracle(ss_ctx, oracle, graph, k_topics):
    """"pr.affine" = 1: every topic from two vectors on k_pr_sweep_n<2>.  Not the reference's operation order: ranks to 1e-12 and equal
    iteration counts, as tests/test_gpu_pagerank.py asserts of this form"""
    n_topic = topic_sizes(graph.n, k_topics)
    for eps, max_iter in MODES:
        with ss_ctx.options(pr__affine=1):
            got = graph.pagerank(D, eps, n_topic, max_iter=max_iter)
        assert_meets_oracle(oracle, got, k_topics, eps, max_iter)


@pytest.mark.parametrize("world", [2, 3])
def test_shards_in_one_process(ss_ctx, oracle, world):
    """ss_pagerank_run_group on doc-range shards: every rank owns hub pieces and items of every other class for both row classes
    (asserted with the planner in tests/test_pr_class_graph_cpu.py from the deal of tests/graph_layout_model.py)"""
    n, ptr, dst = class_boundary_graph()
    graphs = [engine.Graph(ss_ctx, n, ptr, dst, rank=r, world=world) for r in range(world)]
    try:
        infos = [g.info() for g in graphs]
        assert sum(i.n_rows_local for i in infos) == n and sum(i.n_edges_local for i in infos) == len(dst)
        for k_topics in (16, 5, 2, 1):
            n_topic = topic_sizes(n, k_topics)
            for eps, max_iter in ((1e-9, 0), (1e-30, 3)):
                got = engine.Graph.pagerank_group(graphs, D, eps, n_topic, max_iter=max_iter)
                assert_meets_oracle(oracle, got, k_topics, eps, max_iter, (world, k_topics))
    finally:
        for g in graphs:
            g.close()


# planner options that only move work: item size, the V_QUAD / V_ROWW threshold, the deal, the order a wave walks its classes in
MOVES = [{"pr__item_turns": 1}, {"pr__item_turns": 64}, {"pr__t_quad": 64}, {"pr__deal_global": 0}, {"pr__deal_global": 1}, {"pr__deal_global": 2},
         {"pr__class_order": 12345}]


@pytest.mark.parametrize("opts", MOVES, ids=lambda o: "-".join(f"{k[4:]}={v}" for k, v in o.items()))
@pytest.mark.parametrize("k_topics", [16, 1])
def test_planner_options_only_move_work(ss_ctx, oracle, graph, k_topics, opts):
    n_topic = topic_sizes(graph.n, k_topics)
    for eps, max_iter in ((-1.0, 2), (EPS, 0)):
        default = graph.pagerank(D, eps, n_topic, max_iter=max_iter)
        with ss_ctx.options(**opts):
            got = graph.pagerank(D, eps, n_topic, max_iter=max_iter)
        assert got[1].tolist() == default[1].tolist()
        assert_meets_oracle(oracle, got, k_topics, eps, max_iter, opts)
