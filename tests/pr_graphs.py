"""Graphs and option sets that more than one PageRank test module uses (test infrastructure)."""
import functools

import numpy as np


def csr(n, edges):
    edges = sorted(edges)
    ptr = np.zeros(n + 1, dtype=np.uint64)
    for s, _ in edges:
        ptr[s + 1] += 1
    return np.cumsum(ptr).astype(np.uint64), np.array([d for _, d in edges], dtype=np.uint32)


# the three kernels K <= 2 can run on: k_pr_sweep_n (default), k_pr_sweep padded to 8 topics, k_pr_step
NARROW_VARIANTS = {"wave_items": {}, "padded_8_wide": {"pr__narrow_wave": 0}, "block_items": {"pr__force_narrow": 1}}


def skewed_graph():
    rng = np.random.default_rng(3)
    n = 70000
    edges = {(int(s), 0) for s in range(1, 60001)}                      # hub: 60k in-edges = many W_SEG segments
    edges |= {(int(s), 1) for s in rng.choice(n, 3000, replace=False)}  # several segments at K=1 (128*64 edges each)
    edges |= {(int(s), 2) for s in rng.choice(n, 300, replace=False)}
    edges |= {(int(a), int(b)) for a, b in rng.integers(0, n, size=(50000, 2))}
    return (n,) + csr(n, list(edges))


def chunk_corner_graph(n_linkers=30000):
    """The graph of test_graph_build_chunk_rows (n_linkers = 30000).  ss_graph_create finds the row of every edge slot per 2048-slot
    chunk; this graph hits the corners: rows that start exactly on chunk boundaries, rows spanning several chunks, > 8192 edge-less
    rows inside one chunk in BOTH directions (dangling sources in id order; non-dangling pages nobody links to, which sort to the
    end of their class), an edge count that is a multiple of the chunk, and the last row ending at the last slot.  A shard gets
    every W-th of the n_linkers pages nobody links to: four shards need 40000 of them for 8192 on each."""
    n = 120000
    assert 30000 <= n_linkers <= 40000
    edges = []
    hubs = list(range(100000, 100008))
    for s in range(3):                                             # three sources with exactly 2048 children: rows on chunk boundaries
        edges += [(s, 50000 + j) for j in range(2048)]
    edges += [(3, 20000 + j) for j in range(5000)]                 # a row over several chunks
    # sources 4 .. 29999 have no out-edges (dangling, a 26k-row empty stretch in the out-edge CSR)
    edges += [(s, hubs[s % 8]) for s in range(30000, 30000 + n_linkers)]   # non-dangling pages with no in-edges of their own (50000.. get some)
    edges += [(s, s + 1) for s in range(110000, 110100)]
    fill = (-len(edges)) % 2048
    edges += [(n - 1, 70000 + j) for j in range(fill)]             # the last row ends at the last slot of the last chunk
    assert len(edges) % 2048 == 0 and len(set(edges)) == len(edges)
    return (n,) + csr(n, edges)


CORNER_LINKERS = {1: 30000, 2: 30000, 3: 30000, 4: 40000}        # world -> n_linkers with which every rank bisects a chunk of its in_ptr


def nine_runs_graph(m=701):
    """Exactly nine distinct in-degrees in each class, each of them on at least m nodes or on every rank up to world = 4 — the
    read-back of the in-degree runs (option "graph.readback_runs") then sees 9 runs per class on every rank.  Nine pure sources
    s_0 .. s_8 (in-degree 0); a target of in-degree d has the parents s_0 .. s_(d-1).  Non-dangling: m targets of every in-degree
    1 .. 8 and the sources; each target also links to four sinks.  Dangling: m targets of every in-degree 1 .. 8 and the four sinks
    (in-degree 8 m + 1).  The ids are shuffled, so that no class is a range of ids."""
    deg = np.repeat(np.arange(1, 9), m)                            # the in-degree of target t, for both target groups
    n_t = len(deg)
    src0, n = 0, 9 + 2 * n_t + 4
    a0, b0, z0 = 9, 9 + n_t, 9 + 2 * n_t                           # non-dangling targets, dangling targets, sinks
    src, dst = [], []
    for j in range(8):                                             # source j links to every target of in-degree > j
        t = np.flatnonzero(deg > j)
        src += [np.full(2 * len(t), src0 + j)]
        dst += [a0 + t, b0 + t]
    for z in range(4):
        src += [a0 + np.arange(n_t)]
        dst += [np.full(n_t, z0 + z)]
    src += [np.full(4, 8)]                                         # the ninth source links to the sinks alone
    dst += [z0 + np.arange(4)]
    perm = np.random.default_rng(9).permutation(n)
    src, dst = perm[np.concatenate(src)], perm[np.concatenate(dst)]
    order = np.lexsort((dst, src))
    ptr = np.zeros(n + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(np.bincount(src, minlength=n))
    return n, ptr, dst[order].astype(np.uint32)


def multi_edge_graph():
    """About 2000 nodes; 10 % of the edges appear two to four times, 1 % are self-loops; node n - 2 has itself as its only child,
    node n - 1 the same child five times.  (The crawler makes children unique; the C ABI takes any CSR.)"""
    rng = np.random.default_rng(41)
    n, e = 2000, 9000
    key = np.unique(rng.integers(0, n - 2, size=3 * e) * n + rng.integers(0, n, size=3 * e))
    key = key[key // n != key % n]
    key = rng.permutation(key)[:e]
    src, dst = key // n, key % n
    rep = rng.choice(e, e // 10, replace=False)
    times = rng.integers(1, 4, size=len(rep))                      # 1 .. 3 further copies
    loops = rng.choice(n - 2, e // 100, replace=False)
    src = np.concatenate((src, np.repeat(src[rep], times), loops, [n - 2], [n - 1] * 5))
    dst = np.concatenate((dst, np.repeat(dst[rep], times), loops, [n - 2], [7] * 5))
    order = np.lexsort((dst, src))
    ptr = np.zeros(n + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(np.bincount(src, minlength=n))
    return n, ptr, dst[order].astype(np.uint32)


# ---- one graph with rows of every sweep-kernel row class, on both sides of every threshold, dangling or not ---------------------
# (tests/test_pr_class_graph_cpu.py proves with the planner harness that it reaches what it claims; tests/test_gpu_pr_classes.py runs it)
SEGW, T_MULTI = 2048, 4096
# thresholds of the wave-item kernels from both sides: T_DEG (8 | 9), the chunks-per-row steps up to the last one below T_QUAD of
# k_pr_sweep (128) and of k_pr_sweep_n (256), T_MULTI, and hubs whose last piece is one edge (2 SEGW + 1 = T_MULTI + 1, 3 SEGW + 1)
# or full (3 SEGW).  (1 .. 8 come with the exact-degree runs below.)
CLASS_WAVE_DEGREES = [9, 16, 17, 32, 33, 112, 113, 128, 129, 240, 241, 256, 257, T_MULTI, T_MULTI + 1, 2 * SEGW + 1, 3 * SEGW, 3 * SEGW + 1]
# thresholds of k_pr_step at gw 1 and 2 (NSLOT = 64, 32): T_WAVE = 2 NSLOT, T_SEG = 32 NSLOT, one / two / four pieces of 128 NSLOT
# edges.  (None is too large for the node count: the longest row, 3 * 8192 + 1 parents, is what sets it.)
CLASS_STEP_DEGREES = sorted({v for s in (64, 32) for v in (2 * s - 1, 2 * s, 2 * s + 1, 32 * s - 1, 32 * s, 32 * s + 1, 128 * s, 128 * s + 1, 3 * 128 * s + 1)})
CLASS_RUN_ROWS = {D: 2 * 256 + 1 + D for D in range(1, 9)}          # rows of exactly D in-edges: more than two items of 256, ragged tail
# rows of one and of two 16-edge chunks: with the threshold rows 69 (9 .. 16) and 37 (17 .. 32) rows, more than max_groups * NSLOT
# (64 / 32 at most) and no multiple of 4
CLASS_NCH_FILL = {12: 67, 24: 35}
CLASS_ZERO_ND, CLASS_ZERO_D = 20800, 40                              # rows without in-edges: non-dangling / dangling


def class_degree_multiset():
    """the in-degrees with in-edges that EACH class of class_boundary_graph() holds, falling"""
    deg = CLASS_WAVE_DEGREES + CLASS_STEP_DEGREES
    for D, rows in {**CLASS_RUN_ROWS, **CLASS_NCH_FILL}.items():
        deg = deg + [D] * rows
    return sorted(deg, reverse=True)


@functools.lru_cache(maxsize=None)
def class_boundary_graph(seed=17):
    """About 30k nodes, unique edges, shuffled ids.  Both classes — non-dangling rows and dangling rows — hold class_degree_multiset();
    CLASS_ZERO_ND non-dangling and CLASS_ZERO_D dangling rows have no in-edges.  A row's parents are distinct non-dangling nodes
    (whoever has a child is one) drawn with weights that fall like a power of the node's position, so the out-degrees differ widely:
    after two sweeps no two parents of a row need hold one contribution, and the rows without in-edges (a shared table row per
    out-degree) have more than 64 distinct out-degrees.  Every non-dangling node gets a child: the longest row, drawn last, takes
    those that have none by then."""
    rng = np.random.default_rng(seed)
    degs = class_degree_multiset()
    n_nd, n_d = len(degs) + CLASS_ZERO_ND, len(degs) + CLASS_ZERO_D
    n = n_nd + n_d
    assert n_nd > degs[0]
    w = rng.permutation((np.arange(n_nd) + 20.0) ** -0.9)
    w /= w.sum()
    cum = np.cumsum(w)
    cum[-1] = 1.0
    # rows: (child, in-degree); child ids 0 .. len(degs) - 1 are the non-dangling targets, n_nd .. the dangling ones; longest last
    rows = sorted([(c, m) for c, m in enumerate(degs)] + [(n_nd + c, m) for c, m in enumerate(degs)], key=lambda r: r[1])
    outdeg = np.zeros(n_nd, dtype=np.int64)
    src, dst = [], []
    for i, (child, m) in enumerate(rows):
        if i == len(rows) - 1:                                       # the longest row: everyone still childless, the rest by weight
            forced = np.flatnonzero(outdeg == 0)
            p = w.copy()
            p[forced] = 0.0
            par = np.concatenate((forced, rng.choice(n_nd, m - len(forced), replace=False, p=p / p.sum())))
        elif m > 48:
            par = rng.choice(n_nd, m, replace=False, p=w)
        else:
            par = np.zeros(0, dtype=np.int64)
            while len(par) < m:                                      # with replacement by weight, first appearances kept
                c = np.concatenate((par, np.searchsorted(cum, rng.random(3 * m + 8), side="right")))
                par = c[np.sort(np.unique(c, return_index=True)[1])]
            par = par[:m]
        outdeg[par] += 1
        src.append(par)
        dst.append(np.full(m, child, dtype=np.int64))
    perm = rng.permutation(n)
    src, dst = perm[np.concatenate(src)], perm[np.concatenate(dst)]
    order = np.lexsort((dst, src))
    ptr = np.zeros(n + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(np.bincount(src, minlength=n))
    return n, ptr, dst[order].astype(np.uint32)


def class_degree_tables(n, ptr, dst):
    """-> (nd, d, rows_nd, rows_d): the falling in-degrees of the non-dangling and of the dangling rows, as lists, and the original
    ids in that order (class, in-degree descending, id ascending: the library's row order)"""
    outdeg = np.diff(np.asarray(ptr).astype(np.int64))
    indeg = np.bincount(np.asarray(dst).astype(np.int64), minlength=n)
    order = np.lexsort((np.arange(n), -indeg, outdeg == 0))
    n_nd = int((outdeg > 0).sum())
    return indeg[order[:n_nd]].tolist(), indeg[order[n_nd:]].tolist(), order[:n_nd], order[n_nd:]


def topic_sizes(n, k):
    return [max(1, n // (1 + 5 * j)) for j in range(k)]               # K different sizes: the topics stop at different sweeps


# ---- hand-built deltas for ss_graph_apply_delta (tests/test_gpu_graph_paths.py; predicates checked in test_graph_layout_cpu.py) ----
def rows_of(n, ptr, dst):
    return [dst[int(ptr[v]):int(ptr[v + 1])].copy() for v in range(n)]


def csr_of(rows):
    ptr = np.zeros(len(rows) + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    dst = np.concatenate(rows).astype(np.uint32) if int(ptr[-1]) else np.zeros(0, np.uint32)
    return ptr, dst


def apply_rows(rows, n_new, changed, lists):
    """the updated rows after one delta"""
    rows = list(rows) + [np.zeros(0, np.uint32) for _ in range(n_new - len(rows))]
    for v, l in zip(changed, lists):
        rows[int(v)] = np.asarray(l, dtype=np.uint32)
    return rows


DELTA_N = 40000


def delta_base_rows():
    """node v links to v + 1, 3 v + 7 and v + 1000 (mod n, made unique, ascending); every fourth node is dangling"""
    n = DELTA_N
    v = np.arange(n)
    c = np.sort(np.stack(((v + 1) % n, (3 * v + 7) % n, (v + 1000) % n), axis=1), axis=1)
    return [np.unique(c[i]).astype(np.uint32) if i % 4 != 3 else np.zeros(0, np.uint32) for i in range(n)]


DELTA_SEAM_NAMES = ("long_row", "rows_on_chunk_boundaries", "last_row_ends_on_last_slot", "empty_stretch", "new_page_with_children",
                    "growth_only", "from_and_to_zero_edges")


@functools.lru_cache(maxsize=1)
def delta_seams():
    """name -> (base rows, [(n_nodes_new, changed, new lists), ...]): every delta with `changed` NOT ascending and unique children"""
    n = DELTA_N
    base = delta_base_rows()
    deg = np.array([len(r) for r in base])
    u = lambda *a: np.arange(*a, dtype=np.uint32)
    seams = {}
    # a changed row longer than two chunks
    seams["long_row"] = (base, [(n, [30001, 12345, 777], [u(5, 7), u(100, 5100), u(0)])])
    # rows 20000, 20001, 20002 get 2048 children each; row 19990 gets what puts the first of them on a chunk boundary of the new CSR
    pad = (-(int(deg[:20000].sum()) - int(deg[19990]))) % 2048 or 2048
    seams["rows_on_chunk_boundaries"] = (base, [(n, [20001, 19990, 20002, 20000], [u(1000, 3048), u(pad), u(30000, 32048), u(7, 2055)])])
    # the last node's row ends on the last slot of the last chunk: e_new is a multiple of 2048 (node 5 loses its children)
    k = (-(int(deg.sum()) - int(deg[5]) - int(deg[n - 1]))) % 2048 or 2048
    seams["last_row_ends_on_last_slot"] = (base, [(n, [n - 1, 5], [u(50, 50 + k), u(0)])])
    # 9001 consecutive nodes lose all their children, node 19001 behind them keeps its own
    gone = np.random.default_rng(4).permutation(np.arange(10000, 19001))
    seams["empty_stretch"] = (base, [(n, list(gone), [u(0)] * len(gone))])
    # a brand-new page that arrives with children, in the delta that grows the node set
    seams["new_page_with_children"] = (base, [(n + 50, [n + 7, 100], [np.array([3, n + 1, n + 49], np.uint32), np.array([8, n + 2], np.uint32)])])
    seams["growth_only"] = (base, [(n + 700, [], [])])
    # no edge at all, then some, then none again, then others
    m = 5000
    empty = [np.zeros(0, np.uint32) for _ in range(m)]
    seams["from_and_to_zero_edges"] = (empty, [(m, [4000, 17, 2500], [u(3), u(1000, 3500), u(4999, 5000)]),
                                               (m, [2500, 4000, 17], [u(0), u(0), u(0)]),
                                               (m, [4999, 9], [u(2000, 4100), u(9, 11)])])
    return seams
