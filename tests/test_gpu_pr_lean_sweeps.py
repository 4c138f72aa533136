"""Lean sweeps (option "pr.lean_sweeps", k_pr_sweep<GW, false, true>): in fixed-iteration mode every sweep of a call but its last
two neither loads nor stores ranks, adds up no L1 change and skips the dangling rows.  Nothing a caller can read may notice: a state
created with the option at 1 (default) and one with it at 0 are stepped alike and must agree bit for bit in read() and in every
status field, for one call of m sweeps, for a chain of calls with reads in between and for the one-call driver.  Which sweeps ran
lean is read from the state's launch counter (ss_pr_lean_sweeps), never from timing: the stop-rule mode, teleport sets, the
two-vector form, K <= 2 and the sweeps next to max_iter must launch none.

The graphs are the small ones of the class tests: class_boundary_graph() has rows of every class (cut hubs, long, mid, the
exact-degree runs, edge-less) as non-dangling AND as dangling rows — a dangling row cut into pieces among them —, multi_edge_graph()
has repeated edges, cycle_chords no dangling row at all, bipartite only dangling destinations."""
import numpy as np
import pytest

from spaghettisearch_amd import engine
from tests.pr_graphs import class_boundary_graph, multi_edge_graph, topic_sizes
from tests.test_gpu_pr_shared_rows import g_bipartite, g_cycle_chords

pytestmark = pytest.mark.gpu
D = 0.75
KS = [3, 8, 16]          # K = 3, 8: k_pr_sweep<8>, K = 16: k_pr_sweep<16>
MS = [1, 2, 3, 4, 7]
GRAPHS = {"classes": class_boundary_graph, "multi_edge": multi_edge_graph, "no_dangling": g_cycle_chords, "only_dangling_destinations": g_bipartite}
_graphs = {}


@pytest.fixture(scope="module")
def graphs(ss_ctx):
    def get(name):
        if name not in _graphs:
            n, ptr, dst = GRAPHS[name]()
            _graphs[name] = engine.Graph(ss_ctx, n, ptr, dst)
        return _graphs[name]
    yield get
    for g in _graphs.values():
        g.close()
    _graphs.clear()


def stepped(ctx, g, n_topic, lean, calls, eps=-1.0, max_iter=0, sets=None, **opts):
    """-> ([(ranks, status) behind every call of `calls`], lean launches) of a state created with pr.lean_sweeps = lean"""
    with ctx.options(pr__lean_sweeps=lean, **opts):
        st = engine.PageRankState(g, D, eps, n_topic, max_iter=max_iter)
    try:
        if sets is not None:
            st.set_teleport(sets)
        st.begin()
        seen = []
        for m, read in calls:
            st.step(m)
            seen.append((st.read() if read else None, st.status()))
        return seen, st.lean_sweeps()
    finally:
        st.close()


def assert_same(a, b):
    assert len(a) == len(b)
    for (xa, sa), (xb, sb) in zip(a, b):
        assert (xa is None) == (xb is None)
        if xa is not None:
            assert np.array_equal(xa, xb)
        assert sa["sweeps"] == sb["sweeps"] and sa["n_active"] == sb["n_active"]
        for key in ("iters", "total", "delta"):                       # total: the control block's S
            assert np.array_equal(sa[key], sb[key]), key


@pytest.mark.parametrize("k_topics", KS)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_one_call_of_m_sweeps(ss_ctx, oracle, graphs, name, k_topics):
    g = graphs(name)
    n_topic = topic_sizes(g.n, k_topics)
    for m in MS:
        on, n_on = stepped(ss_ctx, g, n_topic, 1, [(m, True)])
        off, n_off = stepped(ss_ctx, g, n_topic, 0, [(m, True)])
        assert (n_on, n_off) == (max(0, m - 2), 0), m
        assert_same(on, off)
        assert on[0][1]["sweeps"] == m and on[0][1]["iters"].tolist() == [m] * k_topics
    n, ptr, dst = GRAPHS[name]()
    ref, _ = oracle.pagerank(n, ptr, dst, D, -1.0, n_topic, max_iter=MS[-1])
    np.testing.assert_allclose(on[0][0], ref, rtol=1e-12)             # (the gate of tests/test_gpu_pagerank.py)


@pytest.mark.parametrize("k_topics", KS)
@pytest.mark.parametrize("name", ["classes", "multi_edge"])
def test_a_chain_of_calls_with_reads_between(ss_ctx, graphs, name, k_topics):
    g = graphs(name)
    n_topic = topic_sizes(g.n, k_topics)
    calls = [(3, True), (1, False), (5, True)]
    on, n_on = stepped(ss_ctx, g, n_topic, 1, calls)
    off, n_off = stepped(ss_ctx, g, n_topic, 0, calls)
    assert (n_on, n_off) == (1 + 0 + 3, 0)
    assert_same(on, off)
    singles, _ = stepped(ss_ctx, g, n_topic, 1, [(1, False)] * 8 + [(1, True)])
    assert np.array_equal(on[-1][0], singles[-1][0])
    assert_same(on[-1:], singles[-1:])


@pytest.mark.parametrize("k_topics", KS)
def test_the_one_call_driver(ss_ctx, graphs, k_topics):
    """ss_pagerank_run with eps < 0 and max_iter = m: m - 2 lean sweeps, then two full ones; m = 11 spans two of its batches of 8"""
    import torch
    g = graphs("classes")
    n_topic = topic_sizes(g.n, k_topics)
    for m in MS + [11]:
        out = {}
        for lean in (1, 0):
            buf = torch.full((k_topics, g.n), -1.0, dtype=torch.float64, device="cuda")
            with ss_ctx.options(pr__lean_sweeps=lean):
                iters = g.pagerank_dev(D, -1.0, n_topic, buf, max_iter=m)
            ss_ctx.synchronize()
            out[lean] = buf.cpu().numpy(), iters
        assert np.array_equal(out[1][0], out[0][0]), m
        assert out[1][1].tolist() == out[0][1].tolist() == [m] * k_topics
        state, n_lean = stepped(ss_ctx, g, n_topic, 1, [(m, True)])
        assert np.array_equal(out[1][0], state[0][0]) and n_lean == max(0, m - 2)


def test_max_iter_keeps_its_last_two_sweeps_full(ss_ctx, graphs):
    """a fixed-iteration state with max_iter = 5 asked for 20 sweeps stops at 5: sweeps 4 and 5 are full whatever the call's length"""
    g = graphs("classes")
    n_topic = topic_sizes(g.n, 16)
    on, n_on = stepped(ss_ctx, g, n_topic, 1, [(20, True)], max_iter=5)
    off, n_off = stepped(ss_ctx, g, n_topic, 0, [(20, True)], max_iter=5)
    assert (n_on, n_off) == (3, 0)
    assert_same(on, off)
    assert on[0][1]["sweeps"] == 5 and on[0][1]["n_active"] == 0
    # ... and in two calls, the second of which crosses max_iter
    on, n_on = stepped(ss_ctx, g, n_topic, 1, [(2, False), (9, True)], max_iter=5)
    assert n_on == 1                                                   # sweep 3 alone: 1, 2 end a call, 4, 5 end the run
    assert_same(on[-1:], off)


@pytest.mark.parametrize("k_topics", [3, 16])
def test_who_must_not_run_lean(ss_ctx, graphs, k_topics):
    g = graphs("classes")
    n_topic = topic_sizes(g.n, k_topics)
    calls = [(7, True)]
    # the stop rule reads every sweep's L1 change
    eps_on, n = stepped(ss_ctx, g, n_topic, 1, calls, eps=1e-6)
    assert n == 0
    assert_same(eps_on, stepped(ss_ctx, g, n_topic, 0, calls, eps=1e-6)[0])
    # teleport sets: k_pr_sweep<GW, true> has no lean form
    rng = np.random.default_rng(5)
    sets = [np.sort(rng.choice(g.n, 30 + 7 * k, replace=False)).astype(np.uint32) if k % 3 != 2 else np.zeros(0, np.uint32) for k in range(k_topics)]
    ts_on, n = stepped(ss_ctx, g, n_topic, 1, calls, sets=sets)
    assert n == 0
    assert_same(ts_on, stepped(ss_ctx, g, n_topic, 0, calls, sets=sets)[0])
    # a state created under the two-vector form's option
    _, n = stepped(ss_ctx, g, n_topic, 1, calls, pr__affine=1)
    assert n == 0
    # the option at 0, and the kernels of K <= 2
    assert stepped(ss_ctx, g, n_topic, 0, calls)[1] == 0
    assert stepped(ss_ctx, g, topic_sizes(g.n, 2), 1, calls)[1] == 0
    assert stepped(ss_ctx, g, topic_sizes(g.n, 1), 1, calls, pr__force_narrow=1)[1] == 0


def test_one_topic_padded_to_the_wide_sweep(ss_ctx, graphs):
    """K = 1 on k_pr_sweep<8> ("pr.narrow_wave" = 0 on a small graph): seven padding topics, which a lean sweep must leave at 0.0"""
    g = graphs("multi_edge")
    n_topic = topic_sizes(g.n, 1)
    on, n_on = stepped(ss_ctx, g, n_topic, 1, [(7, True)], pr__narrow_wave=0)
    off, n_off = stepped(ss_ctx, g, n_topic, 0, [(7, True)], pr__narrow_wave=0)
    assert (n_on, n_off) == (5, 0)
    assert_same(on, off)
