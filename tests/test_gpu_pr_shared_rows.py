"""Shared table rows for the edge-less sources (option "pr.share_zero_rows", k_pr_sweep): a non-dangling row without in-edges has
no table row of its own, its in-edge sources gather the shared row of its out-degree through the state's remapped index stream.
Every graph is run with the option at 1 (default) and at 0 (a table row per row): ranks, iteration counts and the control block's
S and delta must be bit-identical, and the ranks must agree with the CPU oracle as in tests/test_gpu_pagerank.py (rtol 1e-12,
equal iteration counts)."""
import numpy as np
import pytest

from spaghettisearch_amd import engine

pytestmark = pytest.mark.gpu
D = 0.75
KS = [3, 8, 16]          # both lane-group widths: K = 3, 8 run k_pr_sweep<8>, K = 16 k_pr_sweep<16>


def csr(n, src, dst):
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    order = np.lexsort((dst, src))
    ptr = np.zeros(n + 1, dtype=np.uint64)
    np.add.at(ptr, src + 1, 1)
    return n, np.cumsum(ptr).astype(np.uint64), dst[order].astype(np.uint32)


def g_cycle_chords():
    """every node has in-edges and out-edges: no shared row at all"""
    n = 601
    i = np.arange(n)
    return csr(n, np.concatenate([i, i]), np.concatenate([(i + 1) % n, (i * 7 + 3) % n]))


def g_bipartite():
    """EVERY edge comes from a source without in-edges: pos_nd == 0, the table holds only the zero row and the shared rows"""
    a, b = 300, 517
    rng = np.random.default_rng(1)
    od = 1 + (np.arange(a) % 5)
    src = np.repeat(np.arange(a), od)
    return csr(a + b, src, a + rng.integers(0, b, src.size))


def g_many_degrees():
    """70 distinct out-degrees among the sources without in-edges (more than a wave's lanes), the largest above 256, three rows each;
    their destinations also have ordinary in-edges"""
    degs = list(range(1, 70)) + [300]
    od = np.repeat(degs, 3)
    a, b = od.size, 1500
    rng = np.random.default_rng(2)
    src = np.repeat(np.arange(a), od)
    dst = a + rng.integers(0, b, src.size)
    ring = a + np.arange(b)
    return csr(a + b, np.concatenate([src, ring, ring]), np.concatenate([dst, a + (np.arange(b) + 1) % b, a + (np.arange(b) * 5 + 2) % b]))


def g_repeated_edges():
    """sources without in-edges with several edges to ONE destination (and ordinary sources beside them)"""
    b = 40
    ring = 6 + np.arange(b)
    src = [0] * 5 + [1] * 3 + [1, 2, 2, 3, 4, 4, 4, 5]
    dst = [6] * 5 + [7] * 3 + [6, 6, 6, 9, 9, 9, 10, 11]
    return csr(6 + b, np.concatenate([src, ring]), np.concatenate([dst, 6 + (np.arange(b) + 1) % b]))


def g_mixed_classes():
    """destinations of every row class — <= 2, <= 4, <= 8 in-edges, 9 .. 256, more than 256, one above 4096 — whose in-edges come from
    sources without in-edges AND from ordinary sources (the sources of a row are sorted: the two kinds meet inside a 16-edge turn)"""
    nz, n = 400, 4000
    rng = np.random.default_rng(3)
    o = np.arange(nz, n)
    src, dst = [o], [nz + (o - nz + 1) % (n - nz)]                     # a ring over the ordinary nodes: each has one in-edge, one out-edge
    targets = [2] * 3 + [3, 4, 4] + [5, 7, 8, 8] + [9, 16, 17, 40, 128, 129, 256] + [257, 1000, 2100] + [4200]
    for j, t in enumerate(targets):
        v = nz + 11 * j + 5
        kz = max(1, (t - 1) // 3)                                      # from sources without in-edges (repeats where there are too few)
        ko = t - 1 - kz
        src += [rng.integers(0, nz, kz), rng.integers(nz, n, ko)]
        dst += [np.full(kz, v), np.full(ko, v)]
    src.append(np.arange(nz))                                          # every such source has at least one out-edge
    dst.append(rng.integers(nz, n, nz))
    return csr(n, np.concatenate(src), np.concatenate(dst))


GRAPHS = {"cycle_chords": g_cycle_chords, "bipartite": g_bipartite, "many_degrees": g_many_degrees, "repeated_edges": g_repeated_edges,
          "mixed_classes": g_mixed_classes}
_built = {}


def graph(name):
    if name not in _built:
        _built[name] = GRAPHS[name]()
    return _built[name]


def topic_sizes(n, k):
    return [max(1, n // (1 + 5 * j)) for j in range(k)]               # K different sizes: the topics stop at different sweeps


def run_state(ctx, g, n_topic, share, eps, max_iter, sweeps=None, sets=None):
    """-> (ranks, read_local ranks by original id, status) of a state created with pr.share_zero_rows = share"""
    with ctx.options(pr__share_zero_rows=share):
        st = engine.PageRankState(g, D, eps, n_topic, max_iter=max_iter)
    try:
        if sets is not None:
            st.set_teleport(sets)
        st.begin()
        if sweeps is not None:
            st.step(sweeps)
            s = st.status()
        else:
            s = st.status()
            while s["n_active"] > 0:
                st.step(4)
                s = st.status()
        x = st.read()
        ids, loc = st.read_local()
        by_id = np.full_like(x, np.nan)
        by_id[:, ids] = loc
        return x, by_id, s
    finally:
        st.close()


def assert_same(a, b):
    (xa, la, sa), (xb, lb, sb) = a, b
    assert np.array_equal(xa, xb)
    assert np.array_equal(la, lb)
    assert np.array_equal(sa["iters"], sb["iters"]) and sa["sweeps"] == sb["sweeps"] and sa["n_active"] == sb["n_active"]
    assert np.array_equal(sa["total"], sb["total"])                    # the control block's S
    assert np.array_equal(sa["delta"], sb["delta"])


@pytest.mark.parametrize("k_topics", KS)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_shared_rows_match_a_row_each_and_the_oracle(ss_ctx, oracle, name, k_topics):
    n, ptr, dst = graph(name)
    n_topic = topic_sizes(n, k_topics)
    g = engine.Graph(ss_ctx, n, ptr, dst)
    try:
        # fixed-iteration mode
        for m in (1, 2, 7):
            on = run_state(ss_ctx, g, n_topic, 1, -1.0, 0, sweeps=m)
            off = run_state(ss_ctx, g, n_topic, 0, -1.0, 0, sweeps=m)
            assert_same(on, off)
            ref, ref_it = oracle.pagerank(n, ptr, dst, D, -1.0, n_topic, max_iter=m)
            assert on[2]["iters"].tolist() == [m] * k_topics == ref_it.tolist()
            np.testing.assert_allclose(on[0], ref, rtol=1e-12)
            # read() walks the original ids, read_local() the rows: both must know the rows that have no table row
            assert np.array_equal(on[0], on[1])
        # to convergence: the topics freeze at different sweeps
        on = run_state(ss_ctx, g, n_topic, 1, 1e-6, 0)
        off = run_state(ss_ctx, g, n_topic, 0, 1e-6, 0)
        assert_same(on, off)
        ref, ref_it = oracle.pagerank(n, ptr, dst, D, 1e-6, n_topic)
        assert on[2]["iters"].tolist() == ref_it.tolist()
        np.testing.assert_allclose(on[0], ref, rtol=1e-12)
        assert np.array_equal(on[0], on[1])
    finally:
        g.close()


@pytest.mark.parametrize("k_topics", KS)
def test_rows_without_a_table_row_read_back(ss_ctx, oracle, k_topics):
    """bipartite graph: NO non-dangling row has a table row; read (by original id) and read_local (by row) return their shared rank"""
    n, ptr, dst = graph("bipartite")
    n_topic = topic_sizes(n, k_topics)
    g = engine.Graph(ss_ctx, n, ptr, dst)
    try:
        x, by_id, s = run_state(ss_ctx, g, n_topic, 1, -1.0, 0, sweeps=3)
        ref, _ = oracle.pagerank(n, ptr, dst, D, -1.0, n_topic, max_iter=3)
        outdeg = np.diff(ptr.astype(np.int64))
        sources = np.flatnonzero(outdeg > 0)                           # exactly the rows whose table rows are gone
        assert sources.size == 300
        for out in (x, by_id):
            np.testing.assert_allclose(out[:, sources], ref[:, sources], rtol=1e-12)
            np.testing.assert_allclose(out, ref, rtol=1e-12)
            assert (out[:, sources] == out[:, sources[:1]]).all()      # one value per topic
    finally:
        g.close()


@pytest.mark.parametrize("k_topics", [3, 16])
def test_teleport_sets_take_the_full_table(ss_ctx, k_topics):
    """a state that gets teleport sets runs with a table row per row whatever the option says: created with it at 1 or at 0, the
    results are equal bit for bit"""
    n, ptr, dst = graph("many_degrees")
    n_topic = topic_sizes(n, k_topics)
    rng = np.random.default_rng(4)
    sets = [np.sort(rng.choice(n, 20 + 9 * k, replace=False)).astype(np.uint32) if k % 3 != 2 else np.zeros(0, np.uint32) for k in range(k_topics)]
    g = engine.Graph(ss_ctx, n, ptr, dst)
    try:
        for sweeps, eps in ((2, -1.0), (None, 1e-6)):
            on = run_state(ss_ctx, g, n_topic, 1, eps, 0, sweeps=sweeps, sets=sets)
            off = run_state(ss_ctx, g, n_topic, 0, eps, 0, sweeps=sweeps, sets=sets)
            assert_same(on, off)
            assert np.array_equal(on[0], on[1])
    finally:
        g.close()
