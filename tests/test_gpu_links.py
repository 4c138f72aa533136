"""ss_graph_set_link_key / ss_graph_top_links / ss_graph_hit_links on the GPU, byte for byte against tests/links_model.py.

The row classes are reached on a graph of 2000 nodes with "links.wave_max" = 128 and "links.chunk_edges" = 64: rows of 0, 1, 63, 64,
65, 127, 128, 129 edges and a split row of 300 (five chunks, the last of 44).  The children graph holds those rows as child lists in
an order the test chooses, so a key can put the best candidates into the first chunk, the last chunk, or one into each chunk, and a
duplicate edge can be made to straddle a cut (positions 63 and 64).  The parents graph is its transpose: the same rows as in-edge
lists, whose order inside a row is the library's own — there the three keys and a random one are simply four different keys, and
the cut is straddled by a row in which every parent links three times (three consecutive entries whichever the order; 64 and 128
are no multiples of 3)."""
import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine, synth
from tests import links_model as lm

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
P, CH = lm.PARENTS, lm.CHILDREN
LENS = [0, 1, 63, 64, 65, 127, 128, 129, 300]
N_STAR = 2000
ROW_DUP, ROW_TRIPLE = len(LENS), len(LENS) + 1      # the rows made for the cuts
SMALL = dict(links__wave_max=128, links__chunk_edges=64)


def csr_of(rows):
    ptr = np.zeros(len(rows) + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    dst = np.concatenate([np.asarray(r, np.uint32) for r in rows]) if int(ptr[-1]) else np.zeros(0, np.uint32)
    return ptr, dst.astype(np.uint32)


class G:
    """a graph on the device with the model's edge lists of both directions"""

    def __init__(self, ctx, n, ptr, dst):
        self.n, self.ptr, self.dst = n, ptr, dst
        self.g = engine.Graph(ctx, n, ptr, dst)
        self.lists = {d: lm.edge_lists(n, ptr, dst, d) for d in (P, CH)}

    def want(self, key, d, nodes, m):
        return lm.top_links(self.n, self.ptr, self.dst, key, d, nodes, m, lists=self.lists[d])

    def check(self, key, d, nodes, m):
        self.g.set_link_key(key)
        got = self.g.top_links(np.asarray(nodes, np.uint32), d, m)
        want = self.want(key, d, nodes, m)
        for a, b, what in zip(got, want, ("links", "n_out", "degree")):
            assert a.tobytes() == b.tobytes(), (what, d, m, np.argwhere(a != b)[:5].tolist())
        return got


@pytest.fixture(scope="module")
def rmat(ss_ctx):
    d = np.load(__file__.rsplit("/", 1)[0] + "/golden/pagerank_rmat600.npz")
    g = G(ss_ctx, int(d["n"]), d["out_ptr"], d["out_dst"])
    g.rank = np.ascontiguousarray(d["rank"][0])
    yield g
    g.g.close()


@pytest.fixture(scope="module")
def star(ss_ctx):
    """-> {CH: graph whose rows i < len(LENS) + 2 are the child lists below, P: its transpose}, the child lists"""
    rng = np.random.default_rng(42)
    rows = [[] for _ in range(N_STAR)]
    for i, L in enumerate(LENS):
        rows[i] = rng.choice(np.arange(20, N_STAR), size=L, replace=False).tolist()
    dup = rng.choice(np.arange(20, N_STAR), size=299, replace=False).tolist()
    rows[ROW_DUP] = dup[:64] + [dup[63]] + dup[64:]                      # 300 edges, positions 63 and 64 hold the same child
    rows[ROW_TRIPLE] = [c for c in rng.choice(np.arange(20, N_STAR), size=100, replace=False).tolist() for _ in range(3)]
    ptr, dst = csr_of(rows)
    gc = G(ss_ctx, N_STAR, ptr, dst)
    tptr, tdst = csr_of(gc.lists[P])                                     # the transpose: node u's children = u's parents in gc
    gp = G(ss_ctx, N_STAR, tptr, tdst)
    assert sorted(gp.lists[P][8]) == sorted(rows[8])
    yield {CH: gc, P: gp}, rows
    gc.g.close()
    gp.g.close()


@pytest.mark.parametrize("m", [1, 5, 64])
@pytest.mark.parametrize("d", [P, CH])
def test_whole_small_graph(rmat, d, m):
    nodes = np.arange(rmat.n, dtype=np.uint32)
    for key in (None, rmat.rank, np.full(rmat.n, 0.25)):
        rmat.check(key, d, nodes, m)


def placement_keys(rows, rng):
    big = rows[8]
    keys = {"random": rng.random(N_STAR)}
    for name, best in (("first-chunk", big[:5]), ("last-chunk", big[-5:]), ("one-per-chunk", big[10::64][:5])):
        k = rng.random(N_STAR)
        k[best] = 10.0 + np.arange(len(best))
        keys[name] = k
    return keys


@pytest.mark.parametrize("d", [P, CH])
def test_row_classes(ss_ctx, star, d):
    graphs, rows = star
    nodes = list(range(len(LENS))) + [8, 0, 8]                            # (a row may be asked for more than once)
    with ss_ctx.options(**SMALL):
        for m in (1, 5, 64):
            graphs[d].check(None, d, nodes, m)
        for name, key in placement_keys(rows, np.random.default_rng(7)).items():
            for m in (1, 5, 64):
                got = graphs[d].check(key, d, nodes, m)
            if name != "random":
                assert sorted(key[got[0][8, :5]].tolist()) == [10.0, 11.0, 12.0, 13.0, 14.0]
    graphs[d].check(None, d, nodes, 5)                                    # the same rows unsplit, at the default options


@pytest.mark.parametrize("d", [P, CH])
def test_distinct_across_a_cut(ss_ctx, star, d):
    graphs, rows = star
    twice = rows[ROW_DUP][63]
    assert rows[ROW_DUP][64] == twice
    rng = np.random.default_rng(3)
    with ss_ctx.options(**SMALL):
        key = rng.random(N_STAR)
        key[twice] = 5.0                                                  # it would win in chunk 0 and in chunk 1
        for m in (1, 2, 5, 64):
            got = graphs[d].check(key, d, [ROW_DUP, ROW_TRIPLE], m)
            assert got[0][0, 0] == twice and (m == 1 or got[0][0, 1] != twice)
        graphs[d].check(None, d, [ROW_DUP, ROW_TRIPLE], 64)
        for seed in range(4):                                             # the row of triples: 64 of 100 candidates, whoever straddles
            got = graphs[d].check(np.random.default_rng(seed).random(N_STAR), d, [ROW_TRIPLE, ROW_DUP], 64)
            assert len(set(got[0][0].tolist())) == 64
        assert graphs[d].g.top_links(np.array([ROW_DUP, ROW_TRIPLE], np.uint32), d, 1)[2].tolist() == [300, 300]


@pytest.mark.parametrize("d", [P, CH])
def test_zero_nan_and_infinite_keys(ss_ctx, star, d):
    graphs, rows = star
    big = rows[8]
    nodes = [8, 5, 2, 1, 0]
    zeros = np.full(N_STAR, -1.0)
    zeros[big[0::2]] = 0.0
    zeros[big[1::2]] = -0.0                                               # equal keys: the row comes out by id
    mixed = np.random.default_rng(5).random(N_STAR)
    mixed[big[0::3]] = NAN
    inf = np.random.default_rng(6).random(N_STAR)
    inf[big[0::4]] = INF
    inf[big[1::4]] = -INF
    inf[big[2::8]] = NAN
    for opts in (SMALL, {}):
        with ss_ctx.options(**opts):
            for key in (zeros, np.full(N_STAR, NAN), mixed, inf):
                for m in (5, 64):
                    got = graphs[d].check(key, d, nodes, m)
            assert got[0][0, :5].tolist() == sorted(big[0::4])[:5]        # +inf first, by id
    got = graphs[d].check(zeros, d, [8], 64)
    assert got[0][0].tolist() == sorted(big)[:64]


def test_degree_counts_duplicates_and_may_be_null(rmat, star):
    graphs, _ = star
    for d in (P, CH):
        g = graphs[d]
        g.g.set_link_key(None)
        links, n_out, degree = g.g.top_links(np.array([ROW_DUP, ROW_TRIPLE, 0], np.uint32), d, 64)
        assert degree.tolist() == [300, 300, 0] and n_out.tolist() == [64, 64, 0]
        l2, n2, none = g.g.top_links(np.array([ROW_DUP, ROW_TRIPLE, 0], np.uint32), d, 64, want_degree=False)
        assert none is None and l2.tobytes() == links.tobytes() and n2.tobytes() == n_out.tobytes()
    for d in (P, CH):
        _, _, degree = rmat.g.top_links(np.arange(rmat.n, dtype=np.uint32), d, 1)
        assert degree.tolist() == [len(r) for r in rmat.lists[d]]


def hit_rows(docs):
    h = np.zeros(docs.shape, dtype=engine.HIT_DTYPE)
    h["doc"] = docs
    h["final"] = NAN                                                      # only .doc is read
    return h


@pytest.mark.parametrize("d", [P, CH])
def test_ids_outside_the_graph(rmat, d):
    rmat.g.set_link_key(rmat.rank)
    nodes = np.array([5, rmat.n, 0xFFFFFFFF, 6, rmat.n + 7, 0xFFFFFFEF, 7], np.uint32)
    got = rmat.check(rmat.rank, d, nodes, 5)
    assert got[1][[1, 2, 4, 5]].tolist() == [0] * 4 and got[2][[1, 2, 4, 5]].tolist() == [0] * 4
    docs = nodes[:6].reshape(2, 3)
    links = np.full((2, 3, 5), 0xABCD, np.uint32)
    n_out = np.full((2, 3), -9, np.int32)
    degree = np.full((2, 3), 0xEEEE, np.uint32)
    want = lm.hit_links(rmat.n, rmat.ptr, rmat.dst, rmat.rank, d, docs, [3, 3], 5, links.copy(), n_out.copy(), degree.copy(), lists=rmat.lists[d])
    got = rmat.g.hit_links(hit_rows(docs), np.array([3, 3], np.int32), d, 5, out=(links, n_out, degree))
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    assert n_out.tolist() == [[want[1][0, 0], 0, 0], [want[1][1, 0], 0, 0]]


@pytest.mark.parametrize("d", [P, CH])
def test_hits_form_leaves_the_rest_untouched(rmat, d):
    import torch
    rng = np.random.default_rng(11)
    n_q, k, m = 6, 7, 5
    docs = rng.integers(0, rmat.n, size=(n_q, k)).astype(np.uint32)
    hits = hit_rows(docs)
    rmat.g.set_link_key(rmat.rank)

    def run(n_hits, device):
        links = np.full((n_q, k, m), 0xDEAD, np.uint32)
        n_out = np.full((n_q, k), -5, np.int32)
        degree = np.full((n_q, k), 0xBEEF, np.uint32)
        want = lm.hit_links(rmat.n, rmat.ptr, rmat.dst, rmat.rank, d, docs, n_hits, m, links.copy(), n_out.copy(), degree.copy(), lists=rmat.lists[d])
        if device:
            t = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()      # noqa: E731
            o = (t(links.reshape(-1)), t(n_out.reshape(-1)), t(degree.reshape(-1)))
            rmat.g.hit_links(torch.from_numpy(hits.view(np.uint8).reshape(-1)).cuda(), t(np.asarray(n_hits, np.int32)), d, m, out=o, k=k)
            got = [x.cpu().numpy() for x in o]
        else:
            got = rmat.g.hit_links(hits, np.asarray(n_hits, np.int32), d, m, out=(links, n_out, degree))
        for a, b, what in zip(got, want, ("links", "n_out", "degree")):
            assert a.tobytes() == b.tobytes(), (what, device)
        return want

    w = run([0, 1, 3, 7, 2, 7], device=False)
    assert (w[0][0] == 0xDEAD).all() and (w[1][2, 3:] == -5).all() and (w[2][2, 3:] == 0xBEEF).all()
    assert run([0, 1, 3, 7, 2, 7], device=True)[1].tobytes() == w[1].tobytes()
    run([-3, k + 5, 2, 0, 7, 1], device=True)                             # device counts outside 0 .. k are clamped by the kernel
    for bad in (-3, k + 5):                                               # host counts outside 0 .. k are refused, outputs untouched
        links = np.full((n_q, k, m), 0xDEAD, np.uint32)
        n_out = np.full((n_q, k), -5, np.int32)
        degree = np.full((n_q, k), 0xBEEF, np.uint32)
        with pytest.raises(SpaghettiError) as ei:
            rmat.g.hit_links(hits, np.array([1, 2, bad, 1, 1, 1], np.int32), d, m, out=(links, n_out, degree))
        assert ei.value.code == 1
        assert (links == 0xDEAD).all() and (n_out == -5).all() and (degree == 0xBEEF).all()


def test_argument_checks(ss_ctx, rmat):
    lib, h = ss_ctx.lib, rmat.g.h
    INVALID, UNSUPPORTED = 1, 7
    nodes = np.arange(4, dtype=np.uint32)
    hits = hit_rows(np.arange(8, dtype=np.uint32).reshape(2, 4))
    n_hits = np.array([4, 4], np.int32)
    links = np.full(8 * 64, 0x5151, np.uint32)
    n_out = np.full(8, -2, np.int32)
    degree = np.full(8, 0x6161, np.uint32)
    p = lambda a: None if a is None else a.ctypes.data                    # noqa: E731

    def top(g=h, d=P, n=4, nd=nodes, m=5, lo=links, no=n_out, do=degree):
        return lib.ss_graph_top_links(g, d, n, p(nd), m, p(lo), p(no), p(do))

    def hit(g=h, d=P, n_q=2, k=4, hs=hits, nh=n_hits, m=5, lo=links, no=n_out, do=degree):
        return lib.ss_graph_hit_links(g, d, n_q, k, p(hs), p(nh), m, p(lo), p(no), p(do))

    assert lib.ss_graph_set_link_key(None, None) == INVALID
    assert top(g=None) == INVALID and hit(g=None) == INVALID
    for kw in (dict(nd=None), dict(lo=None), dict(no=None), dict(d=2), dict(d=-1), dict(m=0), dict(m=-4)):
        assert top(**kw) == INVALID, kw
    for kw in (dict(hs=None), dict(nh=None), dict(lo=None), dict(no=None), dict(d=2), dict(m=0), dict(k=0), dict(k=-1), dict(n_q=-1)):
        assert hit(**kw) == INVALID, kw
    assert top(m=65) == UNSUPPORTED and hit(m=65) == UNSUPPORTED
    assert hit(k=1025) == UNSUPPORTED
    assert top(n=(1 << 31) // 5 + 1) == UNSUPPORTED                       # n * m >= 2^31; nothing is read
    assert top(n=1 << 31, m=1) == UNSUPPORTED
    assert hit(n_q=1 << 21, k=1024, m=1) == UNSUPPORTED                   # n_q * k * m = 2^31
    assert (links == 0x5151).all() and (n_out == -2).all() and (degree == 0x6161).all()
    # nothing to do: SS_OK whatever the pointers
    assert top(n=0, nd=None, lo=None, no=None, do=None) == 0
    assert hit(n_q=0, hs=None, nh=None, lo=None, no=None, do=None) == 0
    assert (links == 0x5151).all() and (n_out == -2).all() and (degree == 0x6161).all()
    assert top() == 0 and (n_out[:4] >= 0).all() and (n_out[4:] == -2).all()


def test_a_shard_is_unsupported(ss_ctx, rmat):
    shard = engine.Graph(ss_ctx, rmat.n, rmat.ptr, rmat.dst, rank=0, world=2)
    try:
        for d in (P, CH):
            links = np.full(5, 0x77, np.uint32)
            n_out = np.full(1, -1, np.int32)
            with pytest.raises(SpaghettiError) as ei:
                shard.top_links(np.zeros(1, np.uint32), d, 5, out=(links, n_out))
            assert ei.value.code == 7 and (links == 0x77).all() and n_out[0] == -1
            with pytest.raises(SpaghettiError) as ei:
                shard.hit_links(hit_rows(np.zeros((1, 1), np.uint32)), np.ones(1, np.int32), d, 5, out=(links, n_out))
            assert ei.value.code == 7 and (links == 0x77).all() and n_out[0] == -1
    finally:
        shard.close()


@pytest.mark.parametrize("d", [P, CH])
def test_device_pointers_give_the_same_bytes(ss_ctx, star, d):
    import torch
    graphs, rows = star
    g = graphs[d]
    key = np.random.default_rng(9).random(N_STAR)
    key[rows[8][::7]] = NAN
    nodes = np.array(list(range(12)) + [N_STAR + 1, 8, 8], np.uint32)
    with ss_ctx.options(**SMALL):
        for m in (5, 64):
            for kk in (None, key):
                g.g.set_link_key(None if kk is None else torch.from_numpy(kk).cuda())      # a key in device memory
                want = g.want(kk, d, nodes, m)
                host = g.g.top_links(nodes, d, m)
                o = (torch.zeros(len(nodes) * m, dtype=torch.int32, device="cuda"), torch.zeros(len(nodes), dtype=torch.int32, device="cuda"),
                     torch.zeros(len(nodes), dtype=torch.int32, device="cuda"))
                g.g.top_links(torch.from_numpy(nodes.view(np.int32)).cuda(), d, m, out=o)
                for a, b, c in zip(host, o, want):
                    assert a.tobytes() == b.cpu().numpy().tobytes() == c.tobytes()
                # mixed: device ids, host outputs; host ids, a device links array
                mixed = g.g.top_links(torch.from_numpy(nodes.view(np.int32)).cuda(), d, m)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(mixed, want))
                lo = torch.zeros(len(nodes) * m, dtype=torch.int32, device="cuda")
                no, do = np.zeros(len(nodes), np.int32), np.zeros(len(nodes), np.uint32)
                g.g.top_links(nodes, d, m, out=(lo, no, do))
                assert lo.cpu().numpy().tobytes() == want[0].tobytes() and no.tobytes() == want[1].tobytes() and do.tobytes() == want[2].tobytes()


def test_after_a_delta_the_links_are_the_new_graphs_and_the_key_is_gone(ss_ctx):
    n, e = 3000, 14000
    ptr, dst = synth.rmat_graph(n, e, seed=17)
    rows = [dst[int(ptr[v]):int(ptr[v + 1])].tolist() for v in range(n)]
    g = engine.Graph(ss_ctx, n, ptr, dst)
    key = np.random.default_rng(1).random(n)
    g.set_link_key(key)
    nodes = np.arange(n + 1, dtype=np.uint32)
    before = {d: g.top_links(nodes[:n], d, 5) for d in (P, CH)}
    for d in (P, CH):
        want = lm.top_links(n, ptr, dst, key, d, nodes[:n], 5)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before[d], want))
    # a failed delta leaves the key
    with pytest.raises(SpaghettiError):
        g.apply_delta(n + 1, np.array([3], np.uint32), np.array([0, 1], np.uint64), np.array([n + 5], np.uint32))
    for d in (P, CH):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g.top_links(nodes[:n], d, 5), before[d]))
    # node 3 gets a new child list with the new node n, a duplicate and a self-loop; node 4 loses its children
    rows2 = rows + [[]]
    rows2[3] = [n, 7, 7, 3, 2999]
    rows2[4] = []
    nptr, ndst = csr_of([rows2[3], rows2[4]])
    g.apply_delta(n + 1, np.array([3, 4], np.uint32), nptr, ndst)
    ptr2, dst2 = csr_of(rows2)
    fresh = engine.Graph(ss_ctx, n + 1, ptr2, dst2)
    try:
        for d in (P, CH):
            got = g.top_links(nodes, d, 5)                                # the key is cleared: ascending ids
            want = lm.top_links(n + 1, ptr2, dst2, None, d, nodes, 5)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), d
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, fresh.top_links(nodes, d, 5)))
        key2 = np.random.default_rng(2).random(n + 1)
        g.set_link_key(key2)
        fresh.set_link_key(key2)
        for d in (P, CH):
            got = g.top_links(nodes, d, 5)
            want = lm.top_links(n + 1, ptr2, dst2, key2, d, nodes, 5)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), d
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, fresh.top_links(nodes, d, 5)))
    finally:
        fresh.close()
        g.close()


def test_pagerank_is_untouched_and_states_do_not_matter(ss_ctx):
    n, e = 5000, 24000
    ptr, dst = synth.rmat_graph(n, e, seed=11)
    n_topic = synth.topic_sizes(n, 3)
    g = engine.Graph(ss_ctx, n, ptr, dst)
    try:
        rank0, it0 = g.pagerank(0.75, 1e-9, n_topic)
        g.set_link_key(rank0[1])
        nodes = np.arange(n, dtype=np.uint32)
        with ss_ctx.options(**SMALL):
            first = {d: g.top_links(nodes, d, 5) for d in (P, CH)}
        for d in (P, CH):
            want = lm.top_links(n, ptr, dst, rank0[1], d, nodes, 5)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first[d], want)), d
        rank1, it1 = g.pagerank(0.75, 1e-9, n_topic)
        assert rank1.tobytes() == rank0.tobytes() and it1.tolist() == it0.tolist()
        st = engine.PageRankState(g, 0.75, 1e-9, n_topic)                 # a state exists: the key may be set, the links are the same
        try:
            st.begin()
            st.step(3)
            g.set_link_key(rank0[1])
            for d in (P, CH):
                assert all(a.tobytes() == b.tobytes() for a, b in zip(g.top_links(nodes, d, 5), first[d]))
        finally:
            st.close()
        rank2, _ = g.pagerank(0.75, 1e-9, n_topic)
        assert rank2.tobytes() == rank0.tobytes()
    finally:
        g.close()
