"""Plain numpy model of the layout ss_graph_create builds (csrc/graph.hip, csrc/graph.hpp).  No device, no library.

From an out-edge CSR over original ids it restates
  * out-degree, in-degree and class of every node (class 0 = has children, class 1 = dangling);
  * the node order: stable by (class, in-degree descending, id ascending) — k_row_keys and the stable radix sort;
  * the deal (k_assign_ids): sorted position i of a class goes to rank i % W, place i // W of that rank's slice of the class;
  * per rank: cnt_nd / cnt_d real rows, the slice lengths sl_nd (with the 2 + TAIL_SUM_ROWS edge-less tail rows when W > 1) and
    sl_d, the local in_ptr over sl_nd + sl_d rows (k_local_ptr) and e_local;
  * per rank and class: the in-degrees of the real rows run-length encoded (what build() reads back for pr_plan.hpp);
  * the fields of ss_graph_info;
  * for any row-pointer array: per EK_CHUNK-slot chunk the rows r_lo / r_hi that k_chunk_first_rows writes for it.
The predicates at the end say which branch of graph.hip an input selects; a test that claims to reach a branch asserts the
predicate on its own input first."""
from types import SimpleNamespace

import numpy as np

EK_CHUNK = 2048              # graph.hip: TPB * EK_PT
TAIL_SUM_ROWS = 32           # graph.hpp
BISECT_ROWS = 4 * EK_CHUNK   # chunk_rows(): r_hi - r_lo above this takes the bisection per slot
READBACK_RUNS = 8192         # option "graph.readback_runs": default and most


def csr_from_edges(n, src, dst):
    """(parents, children) as arrays -> (out_ptr uint64[n + 1], out_dst uint32[e]), rows by parent, children ascending (duplicates kept)"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    order = np.lexsort((dst, src))
    ptr = np.zeros(n + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(np.bincount(src, minlength=n))
    return ptr, dst[order].astype(np.uint32)


def degrees(n, out_ptr, out_dst):
    """-> (outdeg, indeg, cls) int64[n]; cls 1 = dangling (k_outdeg, the run lengths of the edge sort, k_row_keys)"""
    outdeg = np.diff(np.asarray(out_ptr).astype(np.int64))
    indeg = np.bincount(np.asarray(out_dst).astype(np.int64), minlength=n).astype(np.int64)
    return outdeg, indeg, (outdeg == 0).astype(np.int64)


def node_order(indeg, cls):
    """original ids in sorted order: class, then in-degree descending, then id ascending"""
    return np.lexsort((np.arange(len(indeg)), -indeg, cls))


def rle(a):
    """-> (values, lengths) of the runs of equal neighbours"""
    a = np.asarray(a)
    if len(a) == 0:
        return a[:0], np.zeros(0, dtype=np.int64)
    starts = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1])))
    return a[starts], np.diff(np.concatenate((starts, [len(a)])))


def layout(n, out_ptr, out_dst, rank=0, world=1):
    """everything build() derives for one rank"""
    outdeg, indeg, cls = degrees(n, out_ptr, out_dst)
    order = node_order(indeg, cls)
    n_nd = int((cls == 0).sum())
    n_d = n - n_nd
    tail = 2 + TAIL_SUM_ROWS if world > 1 else 0
    sl_nd = (n_nd + world - 1) // world + tail
    sl_d = (n_d + world - 1) // world
    rows_nd = order[:n_nd][rank::world]            # original ids of this rank's rows, in local row order
    rows_d = order[n_nd:][rank::world]
    cnt_nd, cnt_d = len(rows_nd), len(rows_d)
    assert cnt_nd == (n_nd + world - 1 - rank) // world and cnt_d == (n_d + world - 1 - rank) // world
    local_indeg = np.zeros(sl_nd + sl_d, dtype=np.int64)
    local_indeg[:cnt_nd] = indeg[rows_nd]
    local_indeg[sl_nd:sl_nd + cnt_d] = indeg[rows_d]
    in_ptr = np.concatenate(([0], np.cumsum(local_indeg)))
    runs_nd, runs_d = rle(indeg[rows_nd]), rle(indeg[rows_d])
    max_indeg = max([int(r[0][0]) for r in (runs_nd, runs_d) if len(r[0])], default=0)
    return SimpleNamespace(n=n, e=int(out_ptr[-1]), rank=rank, world=world, outdeg=outdeg, indeg=indeg, cls=cls, order=order,
                           n_nd=n_nd, n_d=n_d, sl_nd=sl_nd, sl_d=sl_d, cnt_nd=cnt_nd, cnt_d=cnt_d, rows_nd=rows_nd, rows_d=rows_d,
                           in_ptr=in_ptr, e_local=int(in_ptr[-1]), runs=(runs_nd, runs_d), max_indeg=max_indeg)


INFO_FIELDS = ("n_nodes", "n_edges", "n_nondangling", "n_rows_local", "n_edges_local", "max_indeg", "rank", "world")


def info(lay):
    """ss_graph_info of a layout, as a dict of INFO_FIELDS (max_indeg is this rank's largest in-degree)"""
    return dict(n_nodes=lay.n, n_edges=lay.e, n_nondangling=lay.n_nd, n_rows_local=lay.cnt_nd + lay.cnt_d, n_edges_local=lay.e_local,
                max_indeg=lay.max_indeg, rank=lay.rank, world=lay.world)


def info_of(gi):
    """the same dict from the library's struct"""
    return {f: int(getattr(gi, f)) for f in INFO_FIELDS}


def chunk_first_rows(ptr):
    """k_chunk_first_rows on a row-pointer array: -> (r_lo, r_hi) int64[chunks]; r_lo[c] is the row that holds slot c * EK_CHUNK,
    r_hi[c] the row that holds the next chunk's first slot, for the last chunk the last row with an edge"""
    ptr = np.asarray(ptr).astype(np.int64)
    e = int(ptr[-1])
    chunks = (e + EK_CHUNK - 1) // EK_CHUNK
    if chunks == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    row = np.searchsorted(ptr, np.arange(chunks) * EK_CHUNK, side="right") - 1     # the largest r with ptr[r] <= slot: never an empty row
    last_row = int(np.flatnonzero(np.diff(ptr) > 0)[-1])
    return row, np.concatenate((row[1:], [last_row]))


# ---- predicates: which path an input selects ------------------------------------------------------------------------------
def more_runs_than(lay, c, s):
    """rank's class c (0 = non-dangling, 1 = dangling) has more than s in-degree runs: build() takes the second copy for it"""
    return len(lay.runs[c][0]) > s


def chunk_on_bisection(ptr):
    """some chunk of the row-pointer array spans more than 4 * EK_CHUNK rows: chunk_rows() bisects per slot there"""
    r_lo, r_hi = chunk_first_rows(ptr)
    return bool(np.any(r_hi - r_lo > BISECT_ROWS))


def rows_on_chunk_boundary(ptr):
    """the rows with an edge whose first slot is a multiple of EK_CHUNK other than slot 0"""
    ptr = np.asarray(ptr).astype(np.int64)
    a, b = ptr[:-1], ptr[1:]
    return np.flatnonzero((b > a) & (a > 0) & (a % EK_CHUNK == 0))


def row_on_chunk_boundary(ptr):
    return len(rows_on_chunk_boundary(ptr)) > 0


def row_spans_chunks(ptr, k=3):
    """some row's slots lie in at least k chunks"""
    ptr = np.asarray(ptr).astype(np.int64)
    a, b = ptr[:-1], ptr[1:]
    full = b > a
    return bool(np.any((b[full] - 1) // EK_CHUNK - a[full] // EK_CHUNK + 1 >= k))
