"""Thin object wrappers over the C ABI (include/spaghetti_rank.h).

Arrays may be numpy arrays (host) or torch tensors (host or device): the library
copies with hipMemcpyDefault, so both kinds of pointer are accepted.  Every call
goes through libspaghetti_rank.so — there is no Python/CPU implementation here.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import SsGraphInfo, SsHit, SsPassage, SsProximity, SsTermMatch, check

HIT_DTYPE = np.dtype([("doc", "<u4"), ("_pad", "<u4"), ("title", "<f8"), ("body", "<f8"),
                      ("pagerank", "<f8"), ("final", "<f8")])

TERM_MATCH_DTYPE = np.dtype([("title_w", "<f4"), ("body_w", "<f4"), ("flags", "<u4"), ("body_pos", "<f4")])   # ss_term_match

PASSAGE_DTYPE = np.dtype([("start", "<f4"), ("last", "<f4"), ("n_distinct", "<u4"), ("n_occ", "<u4"), ("token_mask", "<u8")])   # ss_passage
PROXIMITY_DTYPE = np.dtype([("start", "<f4"), ("end", "<f4"), ("n_present", "<u4"), ("n_occ", "<u4"), ("token_mask", "<u8")])   # ss_proximity

DOC_RANGE_DTYPE = np.dtype([("field", "<i4"), ("_pad", "<i4"), ("lo", "<i8"), ("hi", "<i8")])   # ss_doc_range

VEC_HIT_DTYPE = np.dtype([("doc", "<u4"), ("score", "<i4")])   # ss_vec_hit

GROUP_COUNT_DTYPE = np.dtype([("group", "<u4"), ("count", "<u4")])   # ss_group_count

FIELD_STAT_DTYPE = np.dtype([("min", "<i8"), ("max", "<i8"), ("sum_lo", "<u8"), ("sum_hi", "<i8"), ("count", "<u4"), ("missing", "<u4")])   # ss_field_stat
HIST_TAIL_DTYPE = np.dtype([("below", "<u4"), ("above", "<u4"), ("missing", "<u4"), ("n_match", "<u4")])   # ss_hist_tail

DIV_INFO_DTYPE = np.dtype([("rel", "<i4"), ("sim", "<i4")])     # ss_div_info

TREE_NODE_DTYPE = np.dtype([("feature", "<i4"), ("left", "<u4"), ("right", "<u4"), ("nan_left", "<u4"), ("value", "<f8")])   # ss_tree_node
RANK_N_FEATURES = 15                                            # SS_RANK_N_FEATURES: the columns of Scorer.hit_features

FUSED_DTYPE = np.dtype([("score", "<f8"), ("vec_score", "<i4"), ("lex_rank", "<u2"), ("vec_rank", "<u2")])   # ss_fused
FUSE_RRF, FUSE_WEIGHTED = 0, 1                                  # SS_FUSE_RRF, SS_FUSE_WEIGHTED

_NP2T = {"uint64": "int64", "uint32": "int32"}


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _as(x, dtype: str):
    """Contiguous array of the wanted dtype (numpy or torch), no copy when already right.
    torch has no uint32/uint64 storage: int32/int64 tensors of the same bits are accepted."""
    if x is None:
        return None
    if _is_torch(x):
        import torch
        want = getattr(torch, _NP2T.get(dtype, dtype))
        if x.dtype != want:
            raise TypeError(f"torch tensor has dtype {x.dtype}, expected {want}")
        return x.contiguous()
    return np.ascontiguousarray(x, dtype=np.dtype(dtype))


def _ptr(x) -> Optional[int]:
    if x is None:
        return None
    if _is_torch(x):
        return x.data_ptr()
    return x.ctypes.data


class Context:
    """One per GPU per process (ss_init)."""

    def __init__(self, device_id: int = 0):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.ss_init(device_id, C.byref(h)))
        self.h = h
        self.device_id = device_id
        self._options = {}           # name -> value of the options set through this object (options() restores from it)

    def set_stream(self, hip_stream: Optional[int]) -> None:
        check(self.lib.ss_set_stream(self.h, C.c_void_p(hip_stream)), self.h)
        self._shared_stream = bool(hip_stream)

    def ready(self, *arrays) -> None:
        """Device arrays handed to the library must hold their final contents with respect to the context's stream.
        While the context runs on its own (non-blocking) stream, wait for torch's current stream if any argument is a
        CUDA tensor; with a shared stream (set_stream) ordering is the stream's and nothing is done."""
        if getattr(self, "_shared_stream", False):
            return
        for a in arrays:
            if a is not None and _is_torch(a) and a.is_cuda:
                import torch
                torch.cuda.current_stream(a.device).synchronize()
                return

    def merge_hits(self, parts, n_hits, k: int, doc_base=None, out=None):
        """ss_merge_hits: parts [n_parts][n_q][k] hits (numpy HIT_DTYPE, or a torch uint8 tensor of the same bytes),
        n_hits [n_parts][n_q] int32, doc_base uint32[n_parts] | None -> (hits [n_q][k], n_hits [n_q]).
        out=(hits_buf, n_hits_buf) keeps the result in the given (device) buffers."""
        n_hits = _as(n_hits, "int32")
        n_parts, n_q = int(n_hits.shape[0]), int(n_hits.shape[1])
        doc_base = _as(doc_base, "uint32")
        if _is_torch(parts):
            parts = parts.contiguous()
            have = parts.numel() * parts.element_size()
        else:
            parts = np.ascontiguousarray(parts, dtype=HIT_DTYPE)
            have = parts.nbytes
        if have != n_parts * n_q * k * HIT_DTYPE.itemsize:
            raise ValueError("parts does not hold n_parts*n_q*k hits")
        if out is not None:
            hits, n_out = out
            if hits.numel() * hits.element_size() < n_q * k * HIT_DTYPE.itemsize or n_out.numel() < n_q:
                raise ValueError("output buffers too small")
        else:
            hits = np.zeros((n_q, k), dtype=HIT_DTYPE)
            n_out = np.zeros(n_q, dtype=np.int32)
        self.ready(parts, n_hits, doc_base)
        check(self.lib.ss_merge_hits(self.h, n_q, n_parts, k, _ptr(parts), _ptr(n_hits), _ptr(doc_base), _ptr(hits), _ptr(n_out)), self.h)
        return hits, n_out

    def synchronize(self) -> None:
        check(self.lib.ss_synchronize(self.h), self.h)

    def set_option(self, name: str, value: Optional[int]) -> None:
        """ss_set_option: tuning / diagnostic switch of this context; None restores the default."""
        check(self.lib.ss_set_option(self.h, name.encode(), -(1 << 63) if value is None else int(value)), self.h)
        if value is None:
            self._options.pop(name, None)
        else:
            self._options[name] = int(value)

    def options(self, **kv):
        """Context manager: set options (dots written as double underscores: pr__force_narrow=1); on exit every option gets back
        the value it had when the scope was entered (the default if it had none), so scopes nest."""
        ctx = self

        class _Scope:
            def __enter__(self_inner):
                self_inner.before = {k.replace("__", "."): ctx._options.get(k.replace("__", ".")) for k in kv}
                for k, v in kv.items():
                    ctx.set_option(k.replace("__", "."), v)

            def __exit__(self_inner, *exc):
                for name, old in self_inner.before.items():
                    ctx.set_option(name, old)
                return False
        return _Scope()

    # ---- in-library collectives (RCCL over xGMI): one context per rank
    @staticmethod
    def comm_unique_id() -> bytes:
        """ss_comm_unique_id: rank 0 creates the 128-byte id, the host hands it to every rank."""
        buf = C.create_string_buffer(_lib.SS_COMM_ID_BYTES)
        check(_lib.load().ss_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, uid: bytes, rank: int, world: int) -> None:
        if len(uid) != _lib.SS_COMM_ID_BYTES:
            raise ValueError("communicator id must be SS_COMM_ID_BYTES long")
        check(self.lib.ss_comm_init(self.h, C.c_char_p(uid), rank, world), self.h)

    def comm_split(self, color: int, key: int) -> None:
        """ss_comm_split: topic groups x doc shards; the context's communicator becomes its group's."""
        check(self.lib.ss_comm_split(self.h, color, key), self.h)

    def comm_destroy(self) -> None:
        check(self.lib.ss_comm_destroy(self.h), self.h)

    def comm_info(self):
        r, w = C.c_int32(), C.c_int32()
        check(self.lib.ss_comm_info(self.h, C.byref(r), C.byref(w)), self.h)
        return r.value, w.value

    def comm_allreduce_u64(self, buf) -> None:
        """In-place all-reduce(sum) of a uint64 array (numpy host array or torch int64 device tensor)."""
        buf = _as(buf, "uint64")
        self.ready(buf)
        check(self.lib.ss_comm_allreduce_u64(self.h, _ptr(buf), int(buf.shape[0])), self.h)

    def comm_allgather(self, send, recv, bytes_per_rank: int) -> None:
        self.ready(send, recv)
        check(self.lib.ss_comm_allgather(self.h, _ptr(send), _ptr(recv), int(bytes_per_rank)), self.h)

    def last_kernel_ms(self, kind: int) -> float:
        ms = C.c_float(0)
        check(self.lib.ss_last_kernel_ms(self.h, kind, C.byref(ms)), self.h)
        return float(ms.value)

    def close(self) -> None:
        if self.h:
            self.lib.ss_shutdown(self.h)
            self.h = None


class Graph:
    """Link graph (ranking/pagerank.go:17-44) in the library's HBM layout."""

    def __init__(self, ctx: Context, n_nodes: int, out_ptr, out_dst, rank: int = 0, world: int = 1):
        self.ctx = ctx
        self.n = int(n_nodes)
        out_ptr = _as(out_ptr, "uint64")
        out_dst = _as(out_dst, "uint32")
        self.e = int(out_dst.shape[0]) if out_dst is not None else 0
        if out_ptr.shape[0] != self.n + 1:
            raise ValueError("out_ptr must have n_nodes+1 entries")
        ctx.ready(out_ptr, out_dst)
        h = C.c_void_p()
        check(ctx.lib.ss_graph_create(ctx.h, self.n, self.e, _ptr(out_ptr), _ptr(out_dst), rank, world, C.byref(h)), ctx.h)
        self.h = h
        self.rank, self.world = rank, world

    def apply_delta(self, n_nodes_new: int, changed, new_ptr, new_children) -> None:
        """ss_graph_apply_delta: replace the child lists of the `changed` parents (and admit nodes up to n_nodes_new)."""
        changed = _as(changed, "uint32")
        new_ptr = _as(new_ptr, "uint64")
        new_children = _as(new_children, "uint32")
        self.ctx.ready(changed, new_ptr, new_children)
        check(self.ctx.lib.ss_graph_apply_delta(self.h, int(n_nodes_new), int(changed.shape[0]), _ptr(changed), _ptr(new_ptr), _ptr(new_children)),
              self.ctx.h)
        self.n = int(n_nodes_new)

    def info(self) -> SsGraphInfo:
        gi = SsGraphInfo()
        check(self.ctx.lib.ss_graph_get_info(self.h, C.byref(gi)), self.ctx.h)
        return gi

    def pagerank_sharded(self, damping: float, eps: float, n_topic: Sequence[int], max_iter: int = 0, allreduce: bool = False, out=None):
        """ss_pagerank_run_sharded (this rank's part of the doc-range-sharded loop, collectives inside the library):
        -> (ids uint32[rows], rank [K][rows] float64, iters [K] int32).  out = (ids, rank) device tensors keeps the result
        in HBM (torch int32 [rows], float64 [K][rows])."""
        n_topic = np.ascontiguousarray(np.atleast_1d(n_topic), dtype=np.int32)
        K = len(n_topic)
        rows = int(self.info().n_rows_local)
        if out is not None:
            ids, rank = _as(out[0], "uint32"), _as(out[1], "float64")
            count = lambda a: a.numel() if _is_torch(a) else a.size
            if count(ids) < rows or count(rank) < K * rows:
                raise ValueError("out arrays too small")
        else:
            ids = np.zeros(rows, dtype=np.uint32)
            rank = np.zeros((K, rows), dtype=np.float64)
        iters = np.zeros(K, dtype=np.int32)
        check(self.ctx.lib.ss_pagerank_run_sharded(self.h, damping, eps, max_iter, K, _ptr(n_topic), 1 if allreduce else 0,
                                                   _ptr(ids), _ptr(rank), _ptr(iters)), self.ctx.h)
        return ids, rank, iters

    def pagerank(self, damping: float, eps: float, n_topic: Sequence[int], max_iter: int = 0):
        """ss_pagerank_run: -> (rank [K][N] float64, iters [K] int32)."""
        n_topic = np.ascontiguousarray(np.atleast_1d(n_topic), dtype=np.int32)
        K = len(n_topic)
        rank = np.zeros((K, self.n), dtype=np.float64)
        iters = np.zeros(K, dtype=np.int32)
        check(self.ctx.lib.ss_pagerank_run(self.h, damping, eps, max_iter, K, _ptr(n_topic), _ptr(rank), _ptr(iters)),
              self.ctx.h)
        return rank, iters

    @staticmethod
    def pagerank_group(shards, damping: float, eps: float, n_topic: Sequence[int], max_iter: int = 0):
        """ss_pagerank_run_group: all `world` shards of one graph on one context, the library's pipelined (topic-blocked,
        two-stream) sharded loop with in-process copies as the exchange -> (rank [K][N], iters [K])."""
        n_topic = np.ascontiguousarray(np.atleast_1d(n_topic), dtype=np.int32)
        K = len(n_topic)
        ctx = shards[0].ctx
        hs = (C.c_void_p * len(shards))(*[g.h for g in shards])
        rank = np.zeros((K, shards[0].n), dtype=np.float64)
        iters = np.zeros(K, dtype=np.int32)
        check(ctx.lib.ss_pagerank_run_group(hs, len(shards), damping, eps, max_iter, K, _ptr(n_topic), _ptr(rank), _ptr(iters)), ctx.h)
        return rank, iters

    def pagerank_dev(self, damping: float, eps: float, n_topic: Sequence[int], rank_out, max_iter: int = 0):
        """ss_pagerank_run with the ranks left in device memory (`rank_out`: torch float64 [K][N] on the GPU) -> iters [K]."""
        n_topic = np.ascontiguousarray(np.atleast_1d(n_topic), dtype=np.int32)
        K = len(n_topic)
        rank_out = _as(rank_out, "float64")
        if rank_out.numel() < K * self.n:
            raise ValueError("rank_out too small")
        iters = np.zeros(K, dtype=np.int32)
        check(self.ctx.lib.ss_pagerank_run(self.h, damping, eps, max_iter, K, _ptr(n_topic), _ptr(rank_out), _ptr(iters)),
              self.ctx.h)
        return iters

    def set_link_key(self, key) -> None:
        """ss_graph_set_link_key: register the per-node key that orders top_links / hit_links (float64 [n_nodes], numpy or torch;
        copied), or None to clear.  A successful apply_delta clears it."""
        if key is None:
            check(self.ctx.lib.ss_graph_set_link_key(self.h, None), self.ctx.h)
            return
        key = _as(key, "float64")
        if (key.numel() if _is_torch(key) else key.size) < self.n:
            raise ValueError("key must hold n_nodes values")
        self.ctx.ready(key)
        check(self.ctx.lib.ss_graph_set_link_key(self.h, _ptr(key)), self.ctx.h)

    def _links_out(self, rows: int, m: int, want_degree: bool, out):
        count = lambda a: a.numel() if _is_torch(a) else a.size       # noqa: E731
        if out is not None:
            links, n_out, degree = _as(out[0], "uint32"), _as(out[1], "int32"), _as(out[2], "uint32") if len(out) > 2 else None
            if count(links) < rows * m or count(n_out) < rows or (degree is not None and count(degree) < rows):
                raise ValueError("output buffers too small")
            return links, n_out, degree
        return np.zeros(rows * m, dtype=np.uint32), np.zeros(rows, dtype=np.int32), np.zeros(rows, dtype=np.uint32) if want_degree else None

    def top_links(self, nodes, direction: int, m: int = 5, want_degree: bool = True, out=None):
        """ss_graph_top_links: the m best distinct parents (direction = _lib.SS_LINKS_PARENTS) or children (SS_LINKS_CHILDREN) of every
        node of `nodes` by the registered key (descending, then node id; NaN last; ascending id without a key), and the rows' edge
        counts -> (links uint32[n][m], n_out int32[n], degree uint32[n] | None); entries past n_out[i] keep what the array held
        (zeros here).  out = (links, n_out[, degree | None]): the caller's arrays (numpy, or torch int32 device tensors; returned as
        they are); with device nodes and outputs the library only enqueues."""
        nodes = _as(nodes, "uint32")
        n = int(nodes.numel() if _is_torch(nodes) else nodes.size)
        links, n_out, degree = self._links_out(n, int(m), want_degree, out)
        self.ctx.ready(nodes, links, n_out, degree)
        check(self.ctx.lib.ss_graph_top_links(self.h, int(direction), n, _ptr(nodes), int(m), _ptr(links), _ptr(n_out), _ptr(degree)), self.ctx.h)
        if out is None:
            links = links.reshape(n, int(m))
        elif any(_is_torch(a) for a in (links, n_out, degree)) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return links, n_out, degree

    def hit_links(self, hits, n_hits, direction: int, m: int = 5, want_degree: bool = True, out=None, k: Optional[int] = None):
        """ss_graph_hit_links: top_links for the rows of a scoring call, hits[q][j].doc taken as a node id -> (links uint32[n_q][k][m],
        n_out int32[n_q][k], degree uint32[n_q][k] | None).  hits [n_q][k] / n_hits [n_q]: numpy HIT_DTYPE / int32, or the torch uint8 /
        int32 device tensors score_topk's `out` takes; k defaults to what hits holds per query.  Entries behind a query's last hit keep
        what the arrays held.  out as in top_links."""
        n_hits = _as(n_hits, "int32")
        n_q = int(n_hits.numel() if _is_torch(n_hits) else n_hits.size)
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        hits = hits.contiguous() if _is_torch(hits) else np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        if k is None:
            if n_q > 0 and nbytes(hits) % (n_q * HIT_DTYPE.itemsize):
                raise ValueError("hits does not hold n_q rows of whole ss_hit")
            k = nbytes(hits) // (n_q * HIT_DTYPE.itemsize) if n_q > 0 else 1
        elif nbytes(hits) < n_q * int(k) * HIT_DTYPE.itemsize:
            raise ValueError("hits too small")
        k = int(k)
        links, n_out, degree = self._links_out(n_q * k, int(m), want_degree, out)
        self.ctx.ready(hits, n_hits, links, n_out, degree)
        check(self.ctx.lib.ss_graph_hit_links(self.h, int(direction), n_q, k, _ptr(hits), _ptr(n_hits), int(m), _ptr(links), _ptr(n_out),
                                              _ptr(degree)), self.ctx.h)
        if out is None:
            links, n_out = links.reshape(n_q, k, int(m)), n_out.reshape(n_q, k)
            degree = degree.reshape(n_q, k) if degree is not None else None
        elif any(_is_torch(a) for a in (links, n_out, degree)) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()
        return links, n_out, degree

    def close(self) -> None:
        if self.h:
            self.ctx.lib.ss_graph_destroy(self.h)
            self.h = None


class PageRankState:
    """Step-wise power iteration (ss_pr_*), used for timing and by the multi-GPU host."""

    def __init__(self, graph: Graph, damping: float, eps: float, n_topic: Sequence[int], max_iter: int = 0):
        self.g = graph
        self.ctx = graph.ctx
        n_topic = np.ascontiguousarray(np.atleast_1d(n_topic), dtype=np.int32)
        self.k = len(n_topic)
        h = C.c_void_p()
        check(self.ctx.lib.ss_pr_create(graph.h, damping, eps, max_iter, self.k, _ptr(n_topic), C.byref(h)), self.ctx.h)
        self.h = h

    def set_teleport(self, sets) -> None:
        """ss_pr_set_teleport: `sets` = one array of DISTINCT node ids per topic (empty = uniform teleport for that topic),
        or None to restore the reference's uniform teleport.  Opt-in true topic-sensitive PageRank."""
        if sets is None:
            check(self.ctx.lib.ss_pr_set_teleport(self.h, None, None), self.ctx.h)
            return
        if len(sets) != self.k:
            raise ValueError("one teleport set per topic")
        ptr = np.zeros(self.k + 1, dtype=np.uint64)
        ptr[1:] = np.cumsum([len(x) for x in sets])
        nodes = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.uint32) for x in sets]) if int(ptr[-1]) else np.zeros(0, np.uint32))
        check(self.ctx.lib.ss_pr_set_teleport(self.h, _ptr(ptr), _ptr(nodes)), self.ctx.h)

    def begin(self) -> None:
        check(self.ctx.lib.ss_pr_begin(self.h), self.ctx.h)

    def step(self, n_steps: int = 1) -> None:
        check(self.ctx.lib.ss_pr_step(self.h, n_steps), self.ctx.h)

    def lean_sweeps(self) -> int:
        """ss_pr_lean_sweeps: sweeps of this state launched in the lean form so far (option pr.lean_sweeps)."""
        n = C.c_int64(0)
        check(self.ctx.lib.ss_pr_lean_sweeps(self.h, C.byref(n)), self.ctx.h)
        return int(n.value)

    def finalize(self) -> None:
        check(self.ctx.lib.ss_pr_finalize(self.h), self.ctx.h)

    def exchange(self, allreduce: bool = False) -> None:
        """ss_pr_exchange: the per-sweep collective inside the library (needs Context.comm_init)."""
        check(self.ctx.lib.ss_pr_exchange(self.h, 1 if allreduce else 0), self.ctx.h)

    def exchange_buffers(self):
        """-> (send_ptr, send_bytes, recv_ptr, recv_bytes) device pointers."""
        sp, rp = C.c_void_p(), C.c_void_p()
        sb, rb = C.c_uint64(), C.c_uint64()
        check(self.ctx.lib.ss_pr_exchange_buffers(self.h, C.byref(sp), C.byref(sb), C.byref(rp), C.byref(rb)), self.ctx.h)
        return sp.value, sb.value, rp.value, rb.value

    def status(self):
        """-> dict(iters, n_active, sweeps, delta, total); waits for the stream."""
        iters = np.zeros(self.k, dtype=np.int32)
        delta = np.zeros(self.k, dtype=np.float64)
        total = np.zeros(self.k, dtype=np.float64)
        na, sw = C.c_int32(), C.c_int32()
        check(self.ctx.lib.ss_pr_status(self.h, _ptr(iters), C.byref(na), C.byref(sw), _ptr(delta), _ptr(total)), self.ctx.h)
        return {"iters": iters, "n_active": na.value, "sweeps": sw.value, "delta": delta, "total": total}

    def probe(self, mode: int = 0, n_reps: int = 5) -> float:
        """ss_pr_probe: ms per gather-only pass over this graph's index stream (diagnostic)."""
        ms = C.c_float(0)
        check(self.ctx.lib.ss_pr_probe(self.h, mode, n_reps, C.byref(ms)), self.ctx.h)
        return float(ms.value)

    def read(self) -> np.ndarray:
        out = np.zeros((self.k, self.g.n), dtype=np.float64)
        check(self.ctx.lib.ss_pr_read(self.h, _ptr(out)), self.ctx.h)
        return out

    def read_local(self):
        n_rows = int(self.g.info().n_rows_local)
        ids = np.zeros(n_rows, dtype=np.uint32)
        out = np.zeros((self.k, n_rows), dtype=np.float64)
        check(self.ctx.lib.ss_pr_read_local(self.h, _ptr(ids), _ptr(out)), self.ctx.h)
        return ids, out

    def close(self) -> None:
        if self.h:
            self.ctx.lib.ss_pr_destroy(self.h)
            self.h = None


class InvertedIndex:
    """One inverted table (inv[0] title / inv[1] body) — ss_index_*."""

    def __init__(self, ctx: Context, n_docs: int, term_ptr, post_doc, post_tf):
        self.ctx = ctx
        self.n_docs = int(n_docs)
        term_ptr = _as(term_ptr, "uint64")
        post_doc = _as(post_doc, "uint32")
        post_tf = _as(post_tf, "float32")
        self.n_terms = int(term_ptr.shape[0]) - 1
        self.n_post = int(post_doc.shape[0])
        ctx.ready(term_ptr, post_doc, post_tf)
        h = C.c_void_p()
        check(ctx.lib.ss_index_create(ctx.h, self.n_docs, self.n_terms, _ptr(term_ptr), _ptr(post_doc), _ptr(post_tf),
                                      C.byref(h)), ctx.h)
        self.h = h

    def tfidf_build(self, total_docs: int, want_w: bool = True, want_mag: bool = True, want_idf: bool = True):
        """ss_tfidf_build (ranking.UpdateTermWeights): -> (w f32[P] | None, mag f64[N] | None, idf f32[T] | None)."""
        w = np.zeros(self.n_post, dtype=np.float32) if want_w else None
        mag = np.zeros(self.n_docs, dtype=np.float64) if want_mag else None
        idf = np.zeros(self.n_terms, dtype=np.float32) if want_idf else None
        check(self.ctx.lib.ss_tfidf_build(self.h, int(total_docs), _ptr(w), _ptr(mag), _ptr(idf)), self.ctx.h)
        return w, mag, idf

    def apply_delta(self, del_docs=None, del_pairs=None, add=None, add_pos=None) -> None:
        """ss_index_apply_delta(_pos): del_docs uint32[], del_pairs = (terms uint32[], docs uint32[]), add = (terms, docs, weights f32[]),
        add_pos = (pos_ptr uint64[n_add+1], pos float32[]) positional postings of the new postings (tables with positions)."""
        dd = _as(del_docs if del_docs is not None else np.zeros(0, np.uint32), "uint32")
        dt, dp = (_as(del_pairs[0], "uint32"), _as(del_pairs[1], "uint32")) if del_pairs is not None else (np.zeros(0, np.uint32),) * 2
        at, ad, aw = (_as(add[0], "uint32"), _as(add[1], "uint32"), _as(add[2], "float32")) if add is not None else \
            (np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32))
        pp, pv = (_as(add_pos[0], "uint64"), _as(add_pos[1], "float32")) if add_pos is not None else (None, None)
        self.ctx.ready(dd, dt, dp, at, ad, aw, pp, pv)
        check(self.ctx.lib.ss_index_apply_delta_pos(self.h, int(dd.shape[0]), _ptr(dd), int(dt.shape[0]), _ptr(dt), _ptr(dp),
                                                    int(at.shape[0]), _ptr(at), _ptr(ad), _ptr(aw), _ptr(pp), _ptr(pv)), self.ctx.h)
        n_post = C.c_uint64()
        check(self.ctx.lib.ss_index_get_info(self.h, None, None, C.byref(n_post)), self.ctx.h)
        self.n_post = int(n_post.value)

    def resize(self, n_docs: int, n_terms: int) -> None:
        """ss_index_resize: grow the doc and / or term space (new words, new child pages of a re-indexed page)."""
        check(self.ctx.lib.ss_index_resize(self.h, int(n_docs), int(n_terms)), self.ctx.h)
        self.n_docs, self.n_terms = int(n_docs), int(n_terms)

    def read_magnitudes(self, docs) -> np.ndarray:
        docs = _as(docs, "uint32")
        out = np.zeros(int(docs.shape[0]), dtype=np.float64)
        check(self.ctx.lib.ss_index_read_magnitudes(self.h, int(docs.shape[0]), _ptr(docs), _ptr(out)), self.ctx.h)
        return out

    def read_positions(self):
        """-> (pos_ptr uint64[P+1], pos float32[]) as they stand (tables with positional postings)."""
        pp = np.zeros(self.n_post + 1, dtype=np.uint64)
        check(self.ctx.lib.ss_index_read_positions(self.h, _ptr(pp), None), self.ctx.h)
        pv = np.zeros(int(pp[-1]), dtype=np.float32)
        check(self.ctx.lib.ss_index_read_positions(self.h, None, _ptr(pv)), self.ctx.h)
        return pp, pv

    def refresh_magnitudes(self) -> np.ndarray:
        mag = np.zeros(self.n_docs, dtype=np.float64)
        check(self.ctx.lib.ss_index_refresh_magnitudes(self.h, _ptr(mag)), self.ctx.h)
        return mag

    def read(self):
        """-> (term_ptr uint64[T+1], post_doc uint32[P], post_w float32[P]) as the table stands."""
        tp = np.zeros(self.n_terms + 1, dtype=np.uint64)
        pd = np.zeros(self.n_post, dtype=np.uint32)
        pw = np.zeros(self.n_post, dtype=np.float32)
        check(self.ctx.lib.ss_index_read(self.h, _ptr(tp), _ptr(pd), _ptr(pw)), self.ctx.h)
        return tp, pd, pw

    def build_doc_view(self) -> None:
        """ss_index_build_doc_view: the doc-major view of the table as it stands (row d = the terms of doc d, ascending term id, with
        their current weights).  A snapshot: tfidf_build, apply_delta and resize free it."""
        check(self.ctx.lib.ss_index_build_doc_view(self.h), self.ctx.h)

    def drop_doc_view(self) -> None:
        check(self.ctx.lib.ss_index_drop_doc_view(self.h), self.ctx.h)

    def read_doc_view(self):
        """-> (doc_ptr uint64[n_docs+1], doc_term uint32[P], doc_w float32[P]) of the view."""
        dp = np.zeros(self.n_docs + 1, dtype=np.uint64)
        check(self.ctx.lib.ss_index_read_doc_view(self.h, _ptr(dp), None, None), self.ctx.h)
        dt = np.zeros(int(dp[-1]), dtype=np.uint32)
        dw = np.zeros(int(dp[-1]), dtype=np.float32)
        check(self.ctx.lib.ss_index_read_doc_view(self.h, None, _ptr(dt), _ptr(dw)), self.ctx.h)
        return dp, dt, dw

    def doc_top_terms(self, docs, m: int, want_w: bool = True, out=None):
        """ss_index_doc_top_terms: the m heaviest terms of every doc of `docs` (weight descending, then term id; NaN last)
        -> (terms uint32[n][m], w float32[n][m] | None, n_out int32[n]); entries past n_out[i] keep what the arrays held (zeros here).
        out = (terms, w | None, n_out): caller's arrays (numpy, or torch int32 / float32 / int32 device tensors)."""
        docs = _as(docs, "uint32")
        n = int(docs.shape[0])
        if out is not None:
            terms, w, n_out = _as(out[0], "uint32"), _as(out[1], "float32"), _as(out[2], "int32")
            count = lambda a: a.numel() if _is_torch(a) else a.size       # noqa: E731
            if count(terms) < n * m or (w is not None and count(w) < n * m) or count(n_out) < n:
                raise ValueError("output buffers too small")
        else:
            terms = np.zeros((n, m), dtype=np.uint32)
            w = np.zeros((n, m), dtype=np.float32) if want_w else None
            n_out = np.zeros(n, dtype=np.int32)
        self.ctx.ready(docs, terms, w, n_out)
        check(self.ctx.lib.ss_index_doc_top_terms(self.h, n, _ptr(docs), int(m), _ptr(terms), _ptr(w), _ptr(n_out)), self.ctx.h)
        return terms, w, n_out

    def build_signatures(self, n_slots: int = 16) -> None:
        """ss_index_build_signatures: a MinHash signature of n_slots (4, 8, .., 32) uint32 per doc from the doc view's term sets
        (build_doc_view first).  A snapshot of its own: tfidf_build, apply_delta and resize free it, dropping the view does not."""
        check(self.ctx.lib.ss_index_build_signatures(self.h, int(n_slots)), self.ctx.h)

    def drop_signatures(self) -> None:
        check(self.ctx.lib.ss_index_drop_signatures(self.h), self.ctx.h)

    def read_signatures(self, docs, out=None):
        """ss_index_read_signatures: -> sig uint32[n][n_slots], row i = the signature of docs[i] (SS_SIG_EMPTY throughout for a doc
        without body terms).  docs: numpy or torch; out: the caller's array (numpy uint32 or a torch int32 device tensor holding at
        least n * n_slots words), returned as it is."""
        docs = _as(docs, "uint32")
        n = int(docs.numel() if _is_torch(docs) else docs.size)
        n_slots = C.c_int32(0)
        check(self.ctx.lib.ss_index_read_signatures(self.h, 0, None, None, C.byref(n_slots)), self.ctx.h)
        if out is None:
            out = np.zeros((n, n_slots.value), dtype=np.uint32)
        else:
            out = _as(out, "uint32")
            if (out.numel() if _is_torch(out) else out.size) < n * n_slots.value:
                raise ValueError("output buffer too small")
        self.ctx.ready(docs, out)
        check(self.ctx.lib.ss_index_read_signatures(self.h, n, _ptr(docs), _ptr(out), None), self.ctx.h)
        return out

    def set_doc_freq(self, df) -> None:
        """ss_index_set_doc_freq: whole-corpus document frequencies when this table is one doc-range shard
        (uint64[n_terms]; None = local list lengths).  Call before tfidf_build."""
        df = _as(df, "uint64")
        if df is not None and int(df.shape[0]) != self.n_terms:
            raise ValueError("df must hold one entry per term")
        self.ctx.ready(df)
        check(self.ctx.lib.ss_index_set_doc_freq(self.h, _ptr(df)), self.ctx.h)

    def set_positions(self, pos_ptr, pos) -> None:
        """Positional postings (listPos[1:] per posting) for phrase search."""
        pos_ptr = _as(pos_ptr, "uint64")
        pos = _as(pos, "float32")
        self.ctx.ready(pos_ptr, pos)
        check(self.ctx.lib.ss_index_set_positions(self.h, _ptr(pos_ptr), _ptr(pos)), self.ctx.h)

    def set_weighted(self, mag) -> None:
        mag = _as(mag, "float64")
        self.ctx.ready(mag)
        check(self.ctx.lib.ss_index_set_weighted(self.h, _ptr(mag)), self.ctx.h)

    def close(self) -> None:
        if self.h:
            check(self.ctx.lib.ss_index_destroy(self.h), self.ctx.h)
            self.h = None


def pack_doc_masks(sets, n_docs: int) -> np.ndarray:
    """Allow-lists for Scorer.set_doc_masks -> uint32 words [n_masks][(n_docs + 31) // 32], bit (d & 31) of word d >> 5 = doc d.
    `sets`: a list of doc-id arrays (ids outside 0 .. n_docs-1 are an error), or a bool array [n_masks][n_docs]."""
    n_words = (int(n_docs) + 31) // 32
    if isinstance(sets, np.ndarray) and sets.dtype == np.bool_:
        if sets.ndim != 2 or sets.shape[1] != n_docs:
            raise ValueError(f"bool masks must have shape [n_masks][{n_docs}], got {sets.shape}")
        bits = np.zeros((sets.shape[0], n_words * 32), dtype=np.bool_)
        bits[:, :n_docs] = sets
    else:
        bits = np.zeros((len(sets), n_words * 32), dtype=np.bool_)
        for i, docs in enumerate(sets):
            docs = np.asarray(docs, dtype=np.int64).ravel()
            if docs.size and (docs.min() < 0 or docs.max() >= n_docs):
                raise ValueError(f"mask {i}: doc id outside 0 .. {n_docs - 1}")
            bits[i, docs] = True
    return np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(bits.shape[0], n_words).astype(np.uint32)


def pack_doc_ranges(sets):
    """Range clauses for Scorer.doc_field_masks / score_topk_filtered: `sets` is one list of (field, lo, hi) clauses per set or query
    (an empty list: no clause) -> (rng_ptr uint32 [n + 1], clauses DOC_RANGE_DTYPE)."""
    ptr = np.zeros(len(sets) + 1, dtype=np.uint32)
    ptr[1:] = np.cumsum([len(c) for c in sets])
    rng = np.zeros(int(ptr[-1]), dtype=DOC_RANGE_DTYPE)
    flat = [c for cs in sets for c in cs]
    rng["field"] = [c[0] for c in flat]
    rng["lo"] = [c[1] for c in flat]
    rng["hi"] = [c[2] for c in flat]
    return ptr, rng


class Scorer:
    """Batched OR-query cosine scorer + PageRank blend + top-k (ss_score_topk)."""

    def __init__(self, ctx: Context, title: InvertedIndex, body: InvertedIndex):
        self.ctx = ctx
        self.title, self.body = title, body
        h = C.c_void_p()
        check(ctx.lib.ss_scorer_create(ctx.h, title.h, body.h, C.byref(h)), ctx.h)
        self.h = h
        self.k_topics = 0
        self.n_fields = 0
        self.n_masks = 0
        self.vec_dim = 0
        self.n_vec_lists = 0

    def set_prior(self, rank) -> None:
        """rank [K][n_docs] topic-major (ss_pagerank_run layout) or None to clear."""
        if rank is None:
            check(self.ctx.lib.ss_scorer_set_prior(self.h, 0, None), self.ctx.h)
            self.k_topics = 0
            return
        rank = _as(rank, "float64")
        self.k_topics = int(rank.shape[0])
        self.ctx.ready(rank)
        check(self.ctx.lib.ss_scorer_set_prior(self.h, self.k_topics, _ptr(rank)), self.ctx.h)

    def set_doc_masks(self, masks) -> None:
        """ss_scorer_set_doc_masks: register allow-lists (uint32 words [n_masks][(n_docs + 31) // 32] as pack_doc_masks gives,
        numpy or torch), or None / an empty set to clear.  Replaces the previous set once the scorer's outstanding work is done."""
        if masks is None or len(masks) == 0:
            check(self.ctx.lib.ss_scorer_set_doc_masks(self.h, 0, None), self.ctx.h)
            self.n_masks = 0
            return
        masks = _as(masks, "uint32")
        self.ctx.ready(masks)
        check(self.ctx.lib.ss_scorer_set_doc_masks(self.h, int(masks.shape[0]), _ptr(masks)), self.ctx.h)
        self.n_masks = int(masks.shape[0])

    def score_topk_masked(self, q_ptr, q_terms, mask_id, k: int, p_ptr=None, p_terms=None, query_len=None, topic_probs=None, out=None):
        """ss_score_topk_masked: query q's top-k restricted to the docs of allow-list mask_id[q] (-1: unrestricted; None: all -1).
        p_ptr / p_terms: quoted phrases as in score_topk_phrase (None: plain OR queries).  out: device outputs as in score_topk."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        mask_id = _as(mask_id, "int32")
        p_ptr = _as(p_ptr, "uint32")
        p_terms = _as(p_terms, "uint32")
        query_len = _as(query_len, "int32")
        topic_probs = _as(topic_probs, "float64")
        n_q = int(q_ptr.shape[0]) - 1
        self.ctx.ready(q_ptr, q_terms, mask_id, p_ptr, p_terms, query_len, topic_probs)
        if out is not None:
            hits, n_hits = out
            if hits.numel() * hits.element_size() < n_q * k * HIT_DTYPE.itemsize or n_hits.numel() < n_q:
                raise ValueError("output buffers too small")
        else:
            hits, n_hits = np.zeros((n_q, k), dtype=HIT_DTYPE), np.zeros(n_q, dtype=np.int32)
        check(self.ctx.lib.ss_score_topk_masked(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(p_ptr), _ptr(p_terms), _ptr(query_len),
                                                _ptr(topic_probs), _ptr(mask_id), k, _ptr(hits), _ptr(n_hits)), self.ctx.h)
        if out is not None and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return hits, n_hits

    def score_topk_constrained(self, q_ptr, q_terms, k: int, req=None, exc=None, mask_id=None, p_ptr=None, p_terms=None,
                               query_len=None, topic_probs=None, out=None):
        """ss_score_topk_constrained: score_topk_masked where every doc of row q must also contain each REQUIRED term of query q
        (title or body posting) and none of its EXCLUDED terms.  req / exc: (ptr [n_q + 1], terms) pairs or None.  Constraint
        terms only filter (they are not scored).  out: device outputs as in score_topk."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        req_ptr, req_terms = (None, None) if req is None else (_as(req[0], "uint32"), _as(req[1], "uint32"))
        exc_ptr, exc_terms = (None, None) if exc is None else (_as(exc[0], "uint32"), _as(exc[1], "uint32"))
        mask_id = _as(mask_id, "int32")
        p_ptr = _as(p_ptr, "uint32")
        p_terms = _as(p_terms, "uint32")
        query_len = _as(query_len, "int32")
        topic_probs = _as(topic_probs, "float64")
        n_q = int(q_ptr.shape[0]) - 1
        self.ctx.ready(q_ptr, q_terms, req_ptr, req_terms, exc_ptr, exc_terms, mask_id, p_ptr, p_terms, query_len, topic_probs)
        if out is not None:
            hits, n_hits = out
            if hits.numel() * hits.element_size() < n_q * k * HIT_DTYPE.itemsize or n_hits.numel() < n_q:
                raise ValueError("output buffers too small")
        else:
            hits, n_hits = np.zeros((n_q, k), dtype=HIT_DTYPE), np.zeros(n_q, dtype=np.int32)
        check(self.ctx.lib.ss_score_topk_constrained(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(p_ptr), _ptr(p_terms), _ptr(query_len),
                                                     _ptr(topic_probs), _ptr(mask_id), _ptr(req_ptr), _ptr(req_terms), _ptr(exc_ptr),
                                                     _ptr(exc_terms), k, _ptr(hits), _ptr(n_hits)), self.ctx.h)
        if out is not None and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return hits, n_hits

    def score_topk_phrase(self, q_ptr, q_terms, p_ptr, p_terms, k: int, query_len=None, topic_probs=None):
        """ss_score_topk_phrase: OR terms + one concatenated quoted phrase per query."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        p_ptr = _as(p_ptr, "uint32")
        p_terms = _as(p_terms, "uint32")
        query_len = _as(query_len, "int32")
        topic_probs = _as(topic_probs, "float64")
        n_q = int(q_ptr.shape[0]) - 1
        self.ctx.ready(q_ptr, q_terms, p_ptr, p_terms, query_len, topic_probs)
        hits = np.zeros((n_q, k), dtype=HIT_DTYPE)
        n_hits = np.zeros(n_q, dtype=np.int32)
        check(self.ctx.lib.ss_score_topk_phrase(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(p_ptr), _ptr(p_terms),
                                                _ptr(query_len), _ptr(topic_probs), k, hits.ctypes.data, _ptr(n_hits)), self.ctx.h)
        return hits, n_hits

    def score_topk(self, q_ptr, q_terms, k: int, query_len=None, topic_probs=None, out=None):
        """-> (hits [n_q][k] HIT_DTYPE, n_hits [n_q] int32).
        out=(hits_buf, n_hits_buf): optional device-resident outputs (torch uint8 tensor of
        n_q*k*40 bytes and int32 tensor of n_q) — results stay in HBM and `out` is returned."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        query_len = _as(query_len, "int32")
        topic_probs = _as(topic_probs, "float64")
        n_q = int(q_ptr.shape[0]) - 1
        self.ctx.ready(q_ptr, q_terms, query_len, topic_probs)
        if out is not None:
            hits, n_hits = out
            if hits.numel() * hits.element_size() < n_q * k * HIT_DTYPE.itemsize or n_hits.numel() < n_q:
                raise ValueError("output buffers too small")
            check(self.ctx.lib.ss_score_topk(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(query_len), _ptr(topic_probs), k,
                                             _ptr(hits), _ptr(n_hits)), self.ctx.h)
            # device outputs: the library only enqueues (results are ordered on the context's stream).  On a stream shared
            # with the caller that is all that is needed; on the context's own stream wait here.
            if not getattr(self.ctx, "_shared_stream", False):
                self.ctx.synchronize()
            return hits, n_hits
        hits = np.zeros((n_q, k), dtype=HIT_DTYPE)
        n_hits = np.zeros(n_q, dtype=np.int32)
        check(self.ctx.lib.ss_score_topk(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(query_len), _ptr(topic_probs), k,
                                         hits.ctypes.data, _ptr(n_hits)), self.ctx.h)
        return hits, n_hits

    def similar_topk(self, seeds, k: int, m: int = 5, topic_probs=None, mask_id=None, out=None):
        """ss_similar_topk: row q = the top k of the query made of seed doc q's m heaviest body terms, without the seed itself
        (the body table needs its doc view: InvertedIndex.build_doc_view).  mask_id: allow-lists as in score_topk_masked.
        out: device outputs as in score_topk."""
        seeds = _as(seeds, "uint32")
        topic_probs = _as(topic_probs, "float64")
        mask_id = _as(mask_id, "int32")
        n_q = int(seeds.shape[0])
        self.ctx.ready(seeds, topic_probs, mask_id)
        if out is not None:
            hits, n_hits = out
            if hits.numel() * hits.element_size() < n_q * k * HIT_DTYPE.itemsize or n_hits.numel() < n_q:
                raise ValueError("output buffers too small")
        else:
            hits, n_hits = np.zeros((n_q, k), dtype=HIT_DTYPE), np.zeros(n_q, dtype=np.int32)
        check(self.ctx.lib.ss_similar_topk(self.h, n_q, _ptr(seeds), int(m), _ptr(topic_probs), _ptr(mask_id), k, _ptr(hits), _ptr(n_hits)),
              self.ctx.h)
        if out is not None and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return hits, n_hits

    def related_terms(self, q_ptr, q_terms, m: int = 10, k_fb: int = 10, m_doc: int = 5, query_len=None, topic_probs=None, mask_id=None,
                      out=None):
        """ss_related_terms: the m heaviest words the k_fb best pages of every query have in common — each page's m_doc heaviest body
        terms, their weights summed per term in rank order — without the query's own terms (the body table needs its doc view).
        -> (terms uint32[n_q][m], score float64[n_q][m], n_out int32[n_q]); entries past n_out[q] keep what the arrays held (zeros here).
        out = (terms, score | None, n_out): caller's arrays (numpy, or torch int32 / float64 / int32 device tensors); with device
        tensors the library only enqueues."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        query_len = _as(query_len, "int32")
        topic_probs = _as(topic_probs, "float64")
        mask_id = _as(mask_id, "int32")
        n_q = int(q_ptr.shape[0]) - 1
        if out is not None:
            terms, score, n_out = _as(out[0], "uint32"), _as(out[1], "float64"), _as(out[2], "int32")
            count = lambda a: a.numel() if _is_torch(a) else a.size       # noqa: E731
            if count(terms) < n_q * m or (score is not None and count(score) < n_q * m) or count(n_out) < n_q:
                raise ValueError("output buffers too small")
        else:
            terms = np.zeros((n_q, m), dtype=np.uint32)
            score = np.zeros((n_q, m), dtype=np.float64)
            n_out = np.zeros(n_q, dtype=np.int32)
        self.ctx.ready(q_ptr, q_terms, query_len, topic_probs, mask_id, terms, score, n_out)
        check(self.ctx.lib.ss_related_terms(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(query_len), _ptr(topic_probs), _ptr(mask_id),
                                            int(k_fb), int(m_doc), int(m), _ptr(terms), _ptr(score), _ptr(n_out)), self.ctx.h)
        if out is not None and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return terms, score, n_out

    def explain_hits(self, q_ptr, q_terms, hits, n_hits, t_stride: Optional[int] = None, out=None, k: Optional[int] = None):
        """ss_explain_hits: per (hit, query token) the stored title / body weight of the (term, doc) posting, whether it exists, and
        the earliest body position >= 0 -> TERM_MATCH_DTYPE [n_q][k][t_stride].  hits [n_q][k] / n_hits [n_q]: the rows of any scoring
        call (numpy HIT_DTYPE, or the torch uint8 / int32 device tensors score_topk's `out` takes); k defaults to what hits holds per
        query.  t_stride
        defaults to the longest query of the batch.  Entries behind a query's last hit or last token keep what the array held (zeros
        here).  out: the caller's array (numpy TERM_MATCH_DTYPE, or a torch uint8 device tensor of n_q * k * t_stride * 16 bytes,
        returned as it is); with device hits, n_hits and out the library only enqueues."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        n_hits = _as(n_hits, "int32")
        n_q = int(q_ptr.shape[0]) - 1
        self.ctx.ready(q_ptr)
        lens = np.diff(q_ptr.cpu().numpy().astype(np.int64) if _is_torch(q_ptr) else q_ptr.astype(np.int64))
        if t_stride is None:
            t_stride = max(1, int(lens.max())) if n_q > 0 else 1
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        if not _is_torch(hits):
            hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        else:
            hits = hits.contiguous()
        if k is None:
            if n_q > 0 and nbytes(hits) % (n_q * HIT_DTYPE.itemsize):
                raise ValueError("hits does not hold n_q rows of whole ss_hit")
            k = nbytes(hits) // (n_q * HIT_DTYPE.itemsize) if n_q > 0 else 1
        elif nbytes(hits) < n_q * int(k) * HIT_DTYPE.itemsize or (n_hits.numel() if _is_torch(n_hits) else n_hits.size) < n_q:
            raise ValueError("hits / n_hits too small")
        if out is None:
            out = np.zeros((n_q, k, int(t_stride)), dtype=TERM_MATCH_DTYPE)
        elif nbytes(out) < n_q * k * int(t_stride) * TERM_MATCH_DTYPE.itemsize:
            raise ValueError("output buffer too small")
        self.ctx.ready(q_terms, hits, n_hits, out)
        check(self.ctx.lib.ss_explain_hits(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), int(k), _ptr(hits), _ptr(n_hits), int(t_stride),
                                           _ptr(out)), self.ctx.h)
        if _is_torch(out) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return out

    def best_passages(self, q_ptr, q_terms, hits, n_hits, width: int = 20, out=None, k: Optional[int] = None):
        """ss_best_passages: per hit the window of `width` body positions that holds most distinct query terms, then most occurrences,
        then starts earliest -> PASSAGE_DTYPE [n_q][k] (n_occ == 0: the doc has no passage).  hits [n_q][k] / n_hits [n_q]: the rows of
        any scoring call (numpy HIT_DTYPE, or the torch uint8 / int32 device tensors score_topk's `out` takes); k defaults to what hits
        holds per query.  Entries behind a query's last hit keep what the array held (zeros here).  out: the caller's array (numpy
        PASSAGE_DTYPE, or a torch uint8 device tensor of n_q * k * 24 bytes, returned as it is); with device hits, n_hits and out the
        library only enqueues."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        n_hits = _as(n_hits, "int32")
        n_q = int(q_ptr.shape[0]) - 1
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        hits = hits.contiguous() if _is_torch(hits) else np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        if k is None:
            if n_q > 0 and nbytes(hits) % (n_q * HIT_DTYPE.itemsize):
                raise ValueError("hits does not hold n_q rows of whole ss_hit")
            k = nbytes(hits) // (n_q * HIT_DTYPE.itemsize) if n_q > 0 else 1
        elif nbytes(hits) < n_q * int(k) * HIT_DTYPE.itemsize or (n_hits.numel() if _is_torch(n_hits) else n_hits.size) < n_q:
            raise ValueError("hits / n_hits too small")
        if out is None:
            out = np.zeros((n_q, k), dtype=PASSAGE_DTYPE)
        elif nbytes(out) < n_q * k * PASSAGE_DTYPE.itemsize:
            raise ValueError("output buffer too small")
        self.ctx.ready(q_ptr, q_terms, hits, n_hits, out)
        check(self.ctx.lib.ss_best_passages(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), int(k), _ptr(hits), _ptr(n_hits), int(width),
                                            _ptr(out)), self.ctx.h)
        if _is_torch(out) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return out

    def hit_proximity(self, q_ptr, q_terms, hits, n_hits, out=None, k: Optional[int] = None):
        """ss_hit_proximity: per hit the smallest body span that holds every query term the doc has at all -> PROXIMITY_DTYPE [n_q][k]
        (n_present == 0: the doc holds none of the query's terms).  hits / n_hits, k and out as in best_passages (out: numpy
        PROXIMITY_DTYPE, or a torch uint8 device tensor of n_q * k * 24 bytes, returned as it is); with device hits, n_hits and out the
        library only enqueues."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        n_hits = _as(n_hits, "int32")
        n_q = int(q_ptr.shape[0]) - 1
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        hits = hits.contiguous() if _is_torch(hits) else np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        if k is None:
            if n_q > 0 and nbytes(hits) % (n_q * HIT_DTYPE.itemsize):
                raise ValueError("hits does not hold n_q rows of whole ss_hit")
            k = nbytes(hits) // (n_q * HIT_DTYPE.itemsize) if n_q > 0 else 1
        elif nbytes(hits) < n_q * int(k) * HIT_DTYPE.itemsize or (n_hits.numel() if _is_torch(n_hits) else n_hits.size) < n_q:
            raise ValueError("hits / n_hits too small")
        if out is None:
            out = np.zeros((n_q, k), dtype=PROXIMITY_DTYPE)
        elif nbytes(out) < n_q * k * PROXIMITY_DTYPE.itemsize:
            raise ValueError("output buffer too small")
        self.ctx.ready(q_ptr, q_terms, hits, n_hits, out)
        check(self.ctx.lib.ss_hit_proximity(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), int(k), _ptr(hits), _ptr(n_hits), _ptr(out)), self.ctx.h)
        if _is_torch(out) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return out

    def _proximity_out(self, n_q: int, k: int, out, want_scores: bool, want_prox: bool):
        """The four output arrays of the proximity re-ranks: the caller's (hits, n_hits, scores | None, prox | None) or fresh numpy ones."""
        if out is None:
            return (np.zeros((n_q, k), dtype=HIT_DTYPE), np.zeros(n_q, dtype=np.int32),
                    np.zeros((n_q, k), dtype=np.float64) if want_scores else None,
                    np.zeros((n_q, k), dtype=PROXIMITY_DTYPE) if want_prox else None)
        o_hits, o_n, o_sc, o_px = out
        o_n, o_sc = _as(o_n, "int32"), _as(o_sc, "float64")
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        if k > 0 and (nbytes(o_hits) < n_q * k * HIT_DTYPE.itemsize or nbytes(o_n) < n_q * 4 or (o_sc is not None and nbytes(o_sc) < n_q * k * 8)
                      or (o_px is not None and nbytes(o_px) < n_q * k * PROXIMITY_DTYPE.itemsize)):
            raise ValueError("output buffers too small")
        return o_hits, o_n, o_sc, o_px

    def rerank_by_proximity(self, q_ptr, q_terms, hits, n_hits, k: int, w_rank: float = 1.0, w_prox: float = 1.0, first: int = 0,
                            k_in: Optional[int] = None, out=None, want_scores: bool = True, want_prox: bool = True):
        """ss_rerank_hits_by_proximity: every window hits[q][: n_hits[q]] sorted stably by w_rank * final + w_prox * bonus, descending
        (NaN scores behind every number, rows outside the table last), bonus = the closeness of the query's terms in the doc's body
        times the share of the query's terms the doc has; page [first, first + k) -> (hits [n_q][k], n_hits [n_q], scores [n_q][k]
        float64 | None, prox [n_q][k] PROXIMITY_DTYPE | None).  hits / n_hits, k_in as in collapse_hits.  out = (hits, n_hits, scores |
        None, prox | None): the caller's arrays (prox: numpy PROXIMITY_DTYPE or a torch uint8 device tensor), returned as they are;
        with device arrays throughout the library only enqueues."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        hits, n_hits, n_q, k_in = self._window(hits, n_hits, k_in)
        if int(q_ptr.shape[0]) - 1 != n_q:
            raise ValueError(f"{int(q_ptr.shape[0]) - 1} queries for {n_q} windows")
        o_hits, o_n, o_sc, o_px = self._proximity_out(n_q, int(k), out, want_scores, want_prox)
        self.ctx.ready(q_ptr, q_terms, hits, n_hits, o_hits, o_n, o_sc, o_px)
        check(self.ctx.lib.ss_rerank_hits_by_proximity(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), k_in, _ptr(hits), _ptr(n_hits), float(w_rank),
                                                       float(w_prox), int(first), int(k), _ptr(o_hits), _ptr(o_n), _ptr(o_sc), _ptr(o_px)),
              self.ctx.h)
        if _is_torch(o_hits) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return o_hits, o_n, o_sc, o_px

    def score_topk_proximity(self, q_ptr, q_terms, k_window: int, k: int, w_rank: float = 1.0, w_prox: float = 1.0, first: int = 0,
                             query_len=None, topic_probs=None, mask_id=None, out=None, want_scores: bool = True, want_prox: bool = True):
        """ss_score_topk_proximity: rerank_by_proximity applied to the rows score_topk_masked gives at k = k_window, without the window
        leaving the device -> (hits [n_q][k], n_hits [n_q], scores | None, prox | None).  out as in rerank_by_proximity: with device
        arrays the library only enqueues."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        query_len = _as(query_len, "int32")
        topic_probs = _as(topic_probs, "float64")
        mask_id = _as(mask_id, "int32")
        n_q = int(q_ptr.shape[0]) - 1
        o_hits, o_n, o_sc, o_px = self._proximity_out(n_q, int(k), out, want_scores, want_prox)
        self.ctx.ready(q_ptr, q_terms, query_len, topic_probs, mask_id, o_hits, o_n, o_sc, o_px)
        check(self.ctx.lib.ss_score_topk_proximity(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(query_len), _ptr(topic_probs), _ptr(mask_id),
                                                   int(k_window), float(w_rank), float(w_prox), int(first), int(k), _ptr(o_hits), _ptr(o_n),
                                                   _ptr(o_sc), _ptr(o_px)), self.ctx.h)
        if _is_torch(o_hits) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return o_hits, o_n, o_sc, o_px

    def _window_extras(self, n_q: int, k_in: int, prox, vec_scores, query_len):
        """The optional per-row inputs of hit_features / rerank_by_model, checked for size: prox (numpy PROXIMITY_DTYPE or a torch
        uint8 device tensor), vec_scores int32, query_len int32."""
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        if prox is not None:
            prox = prox.contiguous() if _is_torch(prox) else np.ascontiguousarray(prox, dtype=PROXIMITY_DTYPE)
        vec_scores, query_len = _as(vec_scores, "int32"), _as(query_len, "int32")
        if ((prox is not None and nbytes(prox) < n_q * k_in * PROXIMITY_DTYPE.itemsize) or (vec_scores is not None and nbytes(vec_scores) < n_q * k_in * 4)
                or (query_len is not None and nbytes(query_len) < n_q * 4)):
            raise ValueError("prox / vec_scores / query_len too small")
        return prox, vec_scores, query_len

    def hit_features(self, hits, n_hits, prox=None, vec_scores=None, query_len=None, k_in: Optional[int] = None, out=None):
        """ss_hit_features: the feature row of every window row -> float64 [n_q][k_in][RANK_N_FEATURES]: title, body, pagerank, final,
        window position, query length, n_present, span, prox, n_occ, vector score, fields 0..3; NaN where a signal is absent.  hits /
        n_hits, k_in as in collapse_hits; prox as hit_proximity returns it, vec_scores as hit_vector_scores; out: the caller's float64
        array (numpy or torch), returned as it is; entries past n_hits[q] keep what they held; with device arrays throughout the
        library only enqueues."""
        hits, n_hits, n_q, k_in = self._window(hits, n_hits, k_in)
        prox, vec_scores, query_len = self._window_extras(n_q, k_in, prox, vec_scores, query_len)
        if out is None:
            out = np.zeros((n_q, k_in, RANK_N_FEATURES), dtype=np.float64)
        else:
            out = _as(out, "float64")
            if (out.numel() if _is_torch(out) else out.size) < n_q * k_in * RANK_N_FEATURES:
                raise ValueError("output buffer too small")
        self.ctx.ready(hits, n_hits, prox, vec_scores, query_len, out)
        check(self.ctx.lib.ss_hit_features(self.h, n_q, k_in, _ptr(hits), _ptr(n_hits), _ptr(prox), _ptr(vec_scores), _ptr(query_len), _ptr(out)),
              self.ctx.h)
        if _is_torch(out) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return out

    def rerank_by_model(self, model: "RankModel", hits, n_hits, k: int, prox=None, vec_scores=None, query_len=None, first: int = 0,
                        k_in: Optional[int] = None, out=None, want_scores: bool = True):
        """ss_rerank_hits_by_model: every window hits[q][: n_hits[q]] sorted stably by the model's score of the row's hit_features entry,
        descending (NaN scores behind every number, rows outside the table last); page [first, first + k) -> (hits [n_q][k], n_hits
        [n_q], scores [n_q][k] float64 | None).  out = (hits, n_hits, scores | None): the caller's arrays, returned as they are; with
        device arrays throughout the library only enqueues."""
        hits, n_hits, n_q, k_in = self._window(hits, n_hits, k_in)
        prox, vec_scores, query_len = self._window_extras(n_q, k_in, prox, vec_scores, query_len)
        o_hits, o_n, o_sc, _ = self._proximity_out(n_q, int(k), out if out is None else (*out, None), want_scores, False)
        self.ctx.ready(hits, n_hits, prox, vec_scores, query_len, o_hits, o_n, o_sc)
        check(self.ctx.lib.ss_rerank_hits_by_model(self.h, model.h, n_q, k_in, _ptr(hits), _ptr(n_hits), _ptr(prox), _ptr(vec_scores),
                                                   _ptr(query_len), int(first), int(k), _ptr(o_hits), _ptr(o_n), _ptr(o_sc)), self.ctx.h)
        if _is_torch(o_hits) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return o_hits, o_n, o_sc

    def set_doc_groups(self, group) -> None:
        """ss_scorer_set_doc_groups: register the doc -> group table (uint32 [n_docs], numpy or torch; SS_NO_GROUP = never collapsed),
        or None to clear.  Replaces the previous table once the scorer's outstanding work is done."""
        if group is None:
            check(self.ctx.lib.ss_scorer_set_doc_groups(self.h, None), self.ctx.h)
            return
        group = _as(group, "uint32")
        n = group.numel() if _is_torch(group) else group.size
        if n != self.title.n_docs:
            raise ValueError(f"group table holds {n} entries, the scorer has {self.title.n_docs} docs")
        self.ctx.ready(group)
        check(self.ctx.lib.ss_scorer_set_doc_groups(self.h, _ptr(group)), self.ctx.h)

    def _collapse_out(self, n_q: int, k: int, out, want_same: bool, want_kept: bool):
        """The four output arrays of the collapse calls: the caller's (hits, n_hits, same | None, n_kept | None) or fresh numpy ones."""
        if out is None:
            return (np.zeros((n_q, k), dtype=HIT_DTYPE), np.zeros(n_q, dtype=np.int32),
                    np.zeros((n_q, k), dtype=np.uint32) if want_same else None, np.zeros(n_q, dtype=np.int32) if want_kept else None)
        hits, n_hits, same, n_kept = out
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        n_hits, same, n_kept = _as(n_hits, "int32"), _as(same, "uint32"), _as(n_kept, "int32")
        if (nbytes(hits) < n_q * k * HIT_DTYPE.itemsize or nbytes(n_hits) < n_q * 4 or (same is not None and nbytes(same) < n_q * k * 4)
                or (n_kept is not None and nbytes(n_kept) < n_q * 4)):
            raise ValueError("output buffers too small")
        return hits, n_hits, same, n_kept

    def collapse_hits(self, hits, n_hits, g: int, k: int, first: int = 0, k_in: Optional[int] = None, out=None,
                      want_same: bool = True, want_kept: bool = True):
        """ss_collapse_hits: at most g rows per group of every window hits[q][: n_hits[q]], in window order, page [first, first + k)
        of the kept rows -> (hits [n_q][k], n_hits [n_q], same [n_q][k] | None, n_kept [n_q] | None).  hits / n_hits: the rows of any
        scoring call (numpy HIT_DTYPE, or the torch uint8 / int32 device tensors score_topk's `out` takes); k_in defaults to what hits
        holds per query.  Entries behind a row's last hit keep what the arrays held (zeros here).  out = (hits, n_hits, same | None,
        n_kept | None): the caller's arrays, returned as they are; with device arrays throughout the library only enqueues."""
        n_hits = _as(n_hits, "int32")
        n_q = int(n_hits.numel() if _is_torch(n_hits) else n_hits.size)
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        hits = hits.contiguous() if _is_torch(hits) else np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        if k_in is None:
            if n_q > 0 and nbytes(hits) % (n_q * HIT_DTYPE.itemsize):
                raise ValueError("hits does not hold n_q rows of whole ss_hit")
            k_in = nbytes(hits) // (n_q * HIT_DTYPE.itemsize) if n_q > 0 else 1
        elif nbytes(hits) < n_q * int(k_in) * HIT_DTYPE.itemsize:
            raise ValueError("hits too small")
        o_hits, o_n, o_same, o_kept = self._collapse_out(n_q, int(k), out, want_same, want_kept)
        self.ctx.ready(hits, n_hits, o_hits, o_n, o_same, o_kept)
        check(self.ctx.lib.ss_collapse_hits(self.h, n_q, int(k_in), _ptr(hits), _ptr(n_hits), int(g), int(first), int(k), _ptr(o_hits),
                                            _ptr(o_n), _ptr(o_same), _ptr(o_kept)), self.ctx.h)
        if _is_torch(o_hits) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return o_hits, o_n, o_same, o_kept

    def dedup_hits(self, hits, n_hits, min_match: int, k: int, first: int = 0, k_in: Optional[int] = None, out=None,
                   want_similar: bool = True, want_kept: bool = True):
        """ss_dedup_hits: drop the near-duplicate rows of every window hits[q][: n_hits[q]] — a row whose body signature agrees in at
        least min_match slots with an earlier kept row's — and return page [first, first + k) of the kept rows in window order
        -> (hits [n_q][k], n_hits [n_q], similar [n_q][k] | None, n_kept [n_q] | None); similar = the rows of the window a kept row
        leads, itself included.  The body table needs signatures (InvertedIndex.build_signatures).  hits / n_hits, k_in and out as in
        collapse_hits: with device arrays throughout the library only enqueues."""
        n_hits = _as(n_hits, "int32")
        n_q = int(n_hits.numel() if _is_torch(n_hits) else n_hits.size)
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        hits = hits.contiguous() if _is_torch(hits) else np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        if k_in is None:
            if n_q > 0 and nbytes(hits) % (n_q * HIT_DTYPE.itemsize):
                raise ValueError("hits does not hold n_q rows of whole ss_hit")
            k_in = nbytes(hits) // (n_q * HIT_DTYPE.itemsize) if n_q > 0 else 1
        elif nbytes(hits) < n_q * int(k_in) * HIT_DTYPE.itemsize:
            raise ValueError("hits too small")
        o_hits, o_n, o_sim, o_kept = self._collapse_out(n_q, int(k), out, want_similar, want_kept)
        self.ctx.ready(hits, n_hits, o_hits, o_n, o_sim, o_kept)
        check(self.ctx.lib.ss_dedup_hits(self.h, n_q, int(k_in), _ptr(hits), _ptr(n_hits), int(min_match), int(first), int(k),
                                         _ptr(o_hits), _ptr(o_n), _ptr(o_sim), _ptr(o_kept)), self.ctx.h)
        if _is_torch(o_hits) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return o_hits, o_n, o_sim, o_kept

    def score_topk_collapsed(self, q_ptr, q_terms, k_window: int, g: int, k: int, first: int = 0, query_len=None, topic_probs=None,
                             mask_id=None, out=None, want_same: bool = True, want_kept: bool = True):
        """ss_score_topk_collapsed: collapse_hits applied to the rows score_topk_masked gives at k = k_window, without the window
        leaving the device -> (hits [n_q][k], n_hits [n_q], same | None, n_kept | None).  out as in collapse_hits: with device arrays
        the library only enqueues."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        query_len = _as(query_len, "int32")
        topic_probs = _as(topic_probs, "float64")
        mask_id = _as(mask_id, "int32")
        n_q = int(q_ptr.shape[0]) - 1
        o_hits, o_n, o_same, o_kept = self._collapse_out(n_q, int(k), out, want_same, want_kept)
        self.ctx.ready(q_ptr, q_terms, query_len, topic_probs, mask_id, o_hits, o_n, o_same, o_kept)
        check(self.ctx.lib.ss_score_topk_collapsed(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(query_len), _ptr(topic_probs),
                                                   _ptr(mask_id), int(k_window), int(g), int(first), int(k), _ptr(o_hits), _ptr(o_n),
                                                   _ptr(o_same), _ptr(o_kept)), self.ctx.h)
        if _is_torch(o_hits) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return o_hits, o_n, o_same, o_kept

    def set_doc_fields(self, values) -> None:
        """ss_scorer_set_doc_fields: register the per-doc field table (int64 [n_fields][n_docs] field-major, numpy or torch; up to
        SS_MAX_DOC_FIELDS fields), or None to clear.  Replaces the previous table once the scorer's outstanding work is done."""
        if values is None:
            check(self.ctx.lib.ss_scorer_set_doc_fields(self.h, 0, None), self.ctx.h)
            self.n_fields = 0
            return
        values = _as(values, "int64")
        if values.ndim != 2 or int(values.shape[1]) != self.title.n_docs:
            raise ValueError(f"field table must have shape [n_fields][{self.title.n_docs}], got {tuple(values.shape)}")
        self.ctx.ready(values)
        check(self.ctx.lib.ss_scorer_set_doc_fields(self.h, int(values.shape[0]), _ptr(values)), self.ctx.h)
        self.n_fields = int(values.shape[0])

    def doc_field_masks(self, ranges, mask_id=None, out=None):
        """ss_doc_field_masks: allow-lists from range clauses, built on the device -> uint32 words [n_sets][(n_docs + 31) // 32] in
        the layout set_doc_masks takes.  ranges: (rng_ptr [n_sets + 1], DOC_RANGE_DTYPE clauses) as pack_doc_ranges gives; mask_id
        [n_sets]: the registered allow-list a set starts from (-1 / None: every doc).  out: the caller's array (numpy, or a torch
        int32 device tensor), returned as it is."""
        rng_ptr = _as(ranges[0], "uint32")
        rng = np.ascontiguousarray(ranges[1], dtype=DOC_RANGE_DTYPE)
        mask_id = _as(mask_id, "int32")
        n_sets = int(rng_ptr.shape[0]) - 1
        n_words = (self.title.n_docs + 31) // 32
        if out is None:
            out = np.zeros((n_sets, n_words), dtype=np.uint32)
        elif (out.numel() * out.element_size() if _is_torch(out) else out.nbytes) < n_sets * n_words * 4:
            raise ValueError("output buffer too small")
        self.ctx.ready(rng_ptr, mask_id, out)
        check(self.ctx.lib.ss_doc_field_masks(self.h, n_sets, _ptr(rng_ptr), _ptr(rng), _ptr(mask_id), _ptr(out)), self.ctx.h)
        return out

    def score_topk_filtered(self, q_ptr, q_terms, k: int, ranges=None, req=None, exc=None, mask_id=None, p_ptr=None, p_terms=None,
                            query_len=None, topic_probs=None, out=None):
        """ss_score_topk_filtered: score_topk_constrained where every doc of row q must also match each range clause of query q
        (lo <= value[field][doc] <= hi over the table of set_doc_fields).  ranges: (rng_ptr [n_q + 1], DOC_RANGE_DTYPE clauses) as
        pack_doc_ranges gives, or None.  The clauses only filter.  out: device outputs as in score_topk."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        rng_ptr, rng = (None, None) if ranges is None else (_as(ranges[0], "uint32"), np.ascontiguousarray(ranges[1], dtype=DOC_RANGE_DTYPE))
        req_ptr, req_terms = (None, None) if req is None else (_as(req[0], "uint32"), _as(req[1], "uint32"))
        exc_ptr, exc_terms = (None, None) if exc is None else (_as(exc[0], "uint32"), _as(exc[1], "uint32"))
        mask_id = _as(mask_id, "int32")
        p_ptr = _as(p_ptr, "uint32")
        p_terms = _as(p_terms, "uint32")
        query_len = _as(query_len, "int32")
        topic_probs = _as(topic_probs, "float64")
        n_q = int(q_ptr.shape[0]) - 1
        self.ctx.ready(q_ptr, q_terms, req_ptr, req_terms, exc_ptr, exc_terms, mask_id, p_ptr, p_terms, query_len, topic_probs)
        if out is not None:
            hits, n_hits = out
            if hits.numel() * hits.element_size() < n_q * k * HIT_DTYPE.itemsize or n_hits.numel() < n_q:
                raise ValueError("output buffers too small")
        else:
            hits, n_hits = np.zeros((n_q, k), dtype=HIT_DTYPE), np.zeros(n_q, dtype=np.int32)
        check(self.ctx.lib.ss_score_topk_filtered(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(p_ptr), _ptr(p_terms), _ptr(query_len),
                                                  _ptr(topic_probs), _ptr(mask_id), _ptr(req_ptr), _ptr(req_terms), _ptr(exc_ptr),
                                                  _ptr(exc_terms), _ptr(rng_ptr), _ptr(rng), k, _ptr(hits), _ptr(n_hits)), self.ctx.h)
        if out is not None and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return hits, n_hits

    def facet_counts(self, q_ptr, q_terms, ranges=None, req=None, exc=None, mask_id=None, buckets=None, want_masks: bool = True, out=None):
        """ss_facet_counts: per query the number of docs score_topk_filtered would rank for the same q_ptr / q_terms, ranges, req, exc
        and mask_id (no phrase form), the number of them in every registered allow-list, and the number in every bucket ->
        (n_match [n_q], mask_counts [n_q][n_masks] | None, bucket_counts [n_q][n_buckets] | None), uint32.  buckets: DOC_RANGE_DTYPE
        [n_buckets] or a list of (field, lo, hi), shared by the batch, at most SS_MAX_FACET_BUCKETS.  want_masks False (or no mask
        registered): no mask counts.  out = (n_match, mask_counts | None, bucket_counts | None): the caller's arrays (numpy uint32, or
        torch int32 device tensors: with device arrays throughout the call only enqueues), returned as they are."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        rng_ptr, rng = (None, None) if ranges is None else (_as(ranges[0], "uint32"), np.ascontiguousarray(ranges[1], dtype=DOC_RANGE_DTYPE))
        req_ptr, req_terms = (None, None) if req is None else (_as(req[0], "uint32"), _as(req[1], "uint32"))
        exc_ptr, exc_terms = (None, None) if exc is None else (_as(exc[0], "uint32"), _as(exc[1], "uint32"))
        mask_id = _as(mask_id, "int32")
        if buckets is not None and not isinstance(buckets, np.ndarray):
            buckets = pack_doc_ranges([list(buckets)])[1]
        buckets = None if buckets is None else np.ascontiguousarray(buckets, dtype=DOC_RANGE_DTYPE)
        n_b = 0 if buckets is None else int(buckets.shape[0])
        n_q = int(q_ptr.shape[0]) - 1
        n_m = self.n_masks if want_masks else 0
        if out is not None:
            n_match, mask_counts, bucket_counts = out
            nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
            if nbytes(n_match) < n_q * 4 or (mask_counts is not None and nbytes(mask_counts) < n_q * self.n_masks * 4) or \
                    (n_b and (bucket_counts is None or nbytes(bucket_counts) < n_q * n_b * 4)):
                raise ValueError("output buffers too small")
        else:
            n_match = np.zeros(n_q, dtype=np.uint32)
            mask_counts = np.zeros((n_q, n_m), dtype=np.uint32) if n_m else None
            bucket_counts = np.zeros((n_q, n_b), dtype=np.uint32) if n_b else None
        self.ctx.ready(q_ptr, q_terms, req_ptr, req_terms, exc_ptr, exc_terms, mask_id, n_match, mask_counts, bucket_counts)
        check(self.ctx.lib.ss_facet_counts(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(mask_id), _ptr(req_ptr), _ptr(req_terms),
                                           _ptr(exc_ptr), _ptr(exc_terms), _ptr(rng_ptr), _ptr(rng), n_b, _ptr(buckets), _ptr(n_match),
                                           _ptr(mask_counts), _ptr(bucket_counts)), self.ctx.h)
        if _is_torch(n_match) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return n_match, mask_counts, bucket_counts

    def field_topk(self, q_ptr, q_terms, field: int, descending: bool = False, first: int = 0, k: int = 10, ranges=None, req=None, exc=None,
                   mask_id=None, out=None):
        """ss_field_topk: per query the page [first, first + k) of ALL docs facet_counts would count for the same q_ptr / q_terms, ranges,
        req, exc and mask_id, ordered by value[field][doc] (ascending, or descending; equal values by ascending doc id) ->
        (docs uint32 [n_q][k], n_out int32 [n_q], values int64 [n_q][k] | None, n_match uint32 [n_q] | None).  first + k <= SS_MAX_TOPK.
        out = (docs, n_out, values | None, n_match | None): the caller's arrays (numpy, or torch device tensors int32 / int32 / int64 /
        int32: with device arrays throughout the call only enqueues), returned as they are; docs and n_out are what score_docs takes."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        rng_ptr, rng = (None, None) if ranges is None else (_as(ranges[0], "uint32"), np.ascontiguousarray(ranges[1], dtype=DOC_RANGE_DTYPE))
        req_ptr, req_terms = (None, None) if req is None else (_as(req[0], "uint32"), _as(req[1], "uint32"))
        exc_ptr, exc_terms = (None, None) if exc is None else (_as(exc[0], "uint32"), _as(exc[1], "uint32"))
        mask_id = _as(mask_id, "int32")
        n_q = int(q_ptr.shape[0]) - 1
        k = int(k)
        if out is not None:
            docs, n_out, values, n_match = out
            nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
            if k >= 1 and (nbytes(docs) < n_q * k * 4 or nbytes(n_out) < n_q * 4 or (values is not None and nbytes(values) < n_q * k * 8)
                           or (n_match is not None and nbytes(n_match) < n_q * 4)):
                raise ValueError("output buffers too small")
        else:
            docs = np.zeros((n_q, max(k, 0)), dtype=np.uint32)
            n_out = np.zeros(n_q, dtype=np.int32)
            values = np.zeros((n_q, max(k, 0)), dtype=np.int64)
            n_match = np.zeros(n_q, dtype=np.uint32)
        self.ctx.ready(q_ptr, q_terms, req_ptr, req_terms, exc_ptr, exc_terms, mask_id, docs, n_out, values, n_match)
        check(self.ctx.lib.ss_field_topk(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(mask_id), _ptr(req_ptr), _ptr(req_terms), _ptr(exc_ptr),
                                         _ptr(exc_terms), _ptr(rng_ptr), _ptr(rng), int(field), int(bool(descending)), int(first), k,
                                         _ptr(docs), _ptr(n_out), _ptr(values), _ptr(n_match)), self.ctx.h)
        if _is_torch(docs) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return docs, n_out, values, n_match

    def group_values(self) -> np.ndarray:
        """ss_scorer_group_values: the distinct values != SS_NO_GROUP of the registered group table, ascending -> uint32 [n_groups].
        The first call after set_doc_groups builds the group ranks and waits for it."""
        n = C.c_uint32(0)
        check(self.ctx.lib.ss_scorer_group_values(self.h, C.byref(n), None), self.ctx.h)
        values = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            check(self.ctx.lib.ss_scorer_group_values(self.h, None, _ptr(values)), self.ctx.h)
        return values

    def top_groups(self, q_ptr, q_terms, first: int = 0, m: int = 10, ranges=None, req=None, exc=None, mask_id=None, out=None):
        """ss_top_groups: per query the page [first, first + m) of the groups (set_doc_groups) that hold docs facet_counts would count for
        the same q_ptr / q_terms, ranges, req, exc and mask_id, ordered by the number of such docs descending, equal counts by group value
        ascending -> (groups GROUP_COUNT_DTYPE [n_q][m], n_out int32 [n_q], n_groups uint32 [n_q], n_ungrouped uint32 [n_q], n_match
        uint32 [n_q]).  first + m <= SS_MAX_TOPK.  out = (groups, n_out, n_groups | None, n_ungrouped | None, n_match | None): the
        caller's arrays (numpy, or torch device tensors of int32 — groups as [n_q][m][2]: with device arrays throughout, and the group
        ranks built, the call only enqueues), returned as they are."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        rng_ptr, rng = (None, None) if ranges is None else (_as(ranges[0], "uint32"), np.ascontiguousarray(ranges[1], dtype=DOC_RANGE_DTYPE))
        req_ptr, req_terms = (None, None) if req is None else (_as(req[0], "uint32"), _as(req[1], "uint32"))
        exc_ptr, exc_terms = (None, None) if exc is None else (_as(exc[0], "uint32"), _as(exc[1], "uint32"))
        mask_id = _as(mask_id, "int32")
        n_q = int(q_ptr.shape[0]) - 1
        m = int(m)
        if out is not None:
            groups, n_out, n_groups, n_ungrouped, n_match = out
            nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
            if m >= 1 and (nbytes(groups) < n_q * m * GROUP_COUNT_DTYPE.itemsize or nbytes(n_out) < n_q * 4
                           or any(a is not None and nbytes(a) < n_q * 4 for a in (n_groups, n_ungrouped, n_match))):
                raise ValueError("output buffers too small")
        else:
            groups = np.zeros((n_q, max(m, 0)), dtype=GROUP_COUNT_DTYPE)
            n_out = np.zeros(n_q, dtype=np.int32)
            n_groups, n_ungrouped, n_match = (np.zeros(n_q, dtype=np.uint32) for _ in range(3))
        self.ctx.ready(q_ptr, q_terms, req_ptr, req_terms, exc_ptr, exc_terms, mask_id, groups, n_out, n_groups, n_ungrouped, n_match)
        check(self.ctx.lib.ss_top_groups(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(mask_id), _ptr(req_ptr), _ptr(req_terms), _ptr(exc_ptr),
                                         _ptr(exc_terms), _ptr(rng_ptr), _ptr(rng), int(first), m, _ptr(groups), _ptr(n_out), _ptr(n_groups),
                                         _ptr(n_ungrouped), _ptr(n_match)), self.ctx.h)
        if _is_torch(groups) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return groups, n_out, n_groups, n_ungrouped, n_match

    def field_stats(self, q_ptr, q_terms, fields, ranges=None, req=None, exc=None, mask_id=None, out=None):
        """ss_field_stats: per query and per asked field the smallest and largest value, the exact 128-bit sum, and the numbers of docs
        with and without a value (SS_NO_FIELD_VALUE = no value), over ALL docs facet_counts would count for the same q_ptr / q_terms,
        ranges, req, exc and mask_id -> (stats FIELD_STAT_DTYPE [n_q][len(fields)], n_match uint32 [n_q]).  fields: field numbers, at
        most SS_MAX_DOC_FIELDS, repeats allowed.  out = (stats, n_match | None): the caller's arrays (numpy, or torch device tensors —
        stats as int64 [n_q][n][5], n_match int32: with device arrays throughout the call only enqueues), returned as they are."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        rng_ptr, rng = (None, None) if ranges is None else (_as(ranges[0], "uint32"), np.ascontiguousarray(ranges[1], dtype=DOC_RANGE_DTYPE))
        req_ptr, req_terms = (None, None) if req is None else (_as(req[0], "uint32"), _as(req[1], "uint32"))
        exc_ptr, exc_terms = (None, None) if exc is None else (_as(exc[0], "uint32"), _as(exc[1], "uint32"))
        mask_id = _as(mask_id, "int32")
        fields = np.ascontiguousarray(np.atleast_1d(fields), dtype=np.int32)
        n_q, n_f = int(q_ptr.shape[0]) - 1, int(fields.shape[0])
        if out is not None:
            stats, n_match = out
            nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
            if nbytes(stats) < n_q * n_f * FIELD_STAT_DTYPE.itemsize or (n_match is not None and nbytes(n_match) < n_q * 4):
                raise ValueError("output buffers too small")
        else:
            stats = np.zeros((n_q, n_f), dtype=FIELD_STAT_DTYPE)
            n_match = np.zeros(n_q, dtype=np.uint32)
        self.ctx.ready(q_ptr, q_terms, req_ptr, req_terms, exc_ptr, exc_terms, mask_id, stats, n_match)
        check(self.ctx.lib.ss_field_stats(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(mask_id), _ptr(req_ptr), _ptr(req_terms), _ptr(exc_ptr),
                                          _ptr(exc_terms), _ptr(rng_ptr), _ptr(rng), n_f, _ptr(fields) if n_f else None, _ptr(stats),
                                          _ptr(n_match)), self.ctx.h)
        if _is_torch(stats) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return stats, n_match

    def field_histogram(self, q_ptr, q_terms, field: int, n_bins: int, origin: int = 0, width: int = 1, edges=None, ranges=None, req=None,
                        exc=None, mask_id=None, out=None):
        """ss_field_histogram: per query the number of docs facet_counts would count for the same q_ptr / q_terms, ranges, req, exc and
        mask_id in every bin of a field -> (counts uint32 [n_q][n_bins], tails HIST_TAIL_DTYPE [n_q]: below, above, missing, n_match).
        Fixed width (edges None): bin b holds origin + b * width <= value < origin + (b + 1) * width, width in [1, 2^64 - 1].  edges:
        int64 [n_bins + 1] strictly ascending, bin b holds edges[b] <= value < edges[b + 1] (origin and width are ignored).  A doc
        whose value is SS_NO_FIELD_VALUE counts as missing only.  n_bins <= SS_MAX_HIST_BINS.  out = (counts, tails | None): the
        caller's arrays (numpy, or torch device tensors of int32 — tails as [n_q][4]: with device arrays throughout the call only
        enqueues), returned as they are."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        rng_ptr, rng = (None, None) if ranges is None else (_as(ranges[0], "uint32"), np.ascontiguousarray(ranges[1], dtype=DOC_RANGE_DTYPE))
        req_ptr, req_terms = (None, None) if req is None else (_as(req[0], "uint32"), _as(req[1], "uint32"))
        exc_ptr, exc_terms = (None, None) if exc is None else (_as(exc[0], "uint32"), _as(exc[1], "uint32"))
        mask_id = _as(mask_id, "int32")
        edges = None if edges is None else np.ascontiguousarray(edges, dtype=np.int64)
        n_q, n_bins = int(q_ptr.shape[0]) - 1, int(n_bins)
        if edges is not None and n_bins >= 1 and edges.size < n_bins + 1:
            raise ValueError("edges holds fewer than n_bins + 1 values")
        if out is not None:
            counts, tails = out
            nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
            if n_bins >= 1 and (nbytes(counts) < n_q * n_bins * 4 or (tails is not None and nbytes(tails) < n_q * HIST_TAIL_DTYPE.itemsize)):
                raise ValueError("output buffers too small")
        else:
            counts = np.zeros((n_q, max(n_bins, 0)), dtype=np.uint32)
            tails = np.zeros(n_q, dtype=HIST_TAIL_DTYPE)
        self.ctx.ready(q_ptr, q_terms, req_ptr, req_terms, exc_ptr, exc_terms, mask_id, counts, tails)
        check(self.ctx.lib.ss_field_histogram(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(mask_id), _ptr(req_ptr), _ptr(req_terms), _ptr(exc_ptr),
                                              _ptr(exc_terms), _ptr(rng_ptr), _ptr(rng), int(field), int(origin), int(width), _ptr(edges), n_bins,
                                              _ptr(counts), _ptr(tails)), self.ctx.h)
        if _is_torch(counts) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return counts, tails

    def _window(self, hits, n_hits, k_in):
        """(hits, n_hits, n_q, k_in) of a result window as collapse_hits takes it"""
        n_hits = _as(n_hits, "int32")
        n_q = int(n_hits.numel() if _is_torch(n_hits) else n_hits.size)
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        hits = hits.contiguous() if _is_torch(hits) else np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        if k_in is None:
            if n_q > 0 and nbytes(hits) % (n_q * HIT_DTYPE.itemsize):
                raise ValueError("hits does not hold n_q rows of whole ss_hit")
            k_in = nbytes(hits) // (n_q * HIT_DTYPE.itemsize) if n_q > 0 else 1
        elif nbytes(hits) < n_q * int(k_in) * HIT_DTYPE.itemsize:
            raise ValueError("hits too small")
        return hits, n_hits, n_q, int(k_in)

    def sort_hits_by_field(self, hits, n_hits, field: int, k: int, descending: bool = False, first: int = 0,
                           k_in: Optional[int] = None, out=None, want_values: bool = True):
        """ss_sort_hits_by_field: every window hits[q][: n_hits[q]] sorted stably by value[field][doc] (rows outside the table last),
        page [first, first + k) -> (hits [n_q][k], n_hits [n_q], values [n_q][k] int64 | None).  hits / n_hits, k_in as in
        collapse_hits.  out = (hits, n_hits, values | None): the caller's arrays, returned as they are; with device arrays throughout
        the library only enqueues."""
        hits, n_hits, n_q, k_in = self._window(hits, n_hits, k_in)
        if out is None:
            out = (np.zeros((n_q, int(k)), dtype=HIT_DTYPE), np.zeros(n_q, dtype=np.int32),
                   np.zeros((n_q, int(k)), dtype=np.int64) if want_values else None)
        o_hits, o_n, o_vals = out
        o_n, o_vals = _as(o_n, "int32"), _as(o_vals, "int64")
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        if (nbytes(o_hits) < n_q * int(k) * HIT_DTYPE.itemsize or nbytes(o_n) < n_q * 4
                or (o_vals is not None and nbytes(o_vals) < n_q * int(k) * 8)):
            raise ValueError("output buffers too small")
        self.ctx.ready(hits, n_hits, o_hits, o_n, o_vals)
        check(self.ctx.lib.ss_sort_hits_by_field(self.h, n_q, k_in, _ptr(hits), _ptr(n_hits), int(field), int(bool(descending)), int(first),
                                                 int(k), _ptr(o_hits), _ptr(o_n), _ptr(o_vals)), self.ctx.h)
        if _is_torch(o_hits) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return o_hits, o_n, o_vals

    def hit_fields(self, hits, n_hits, k_in: Optional[int] = None, out=None):
        """ss_hit_fields: the field values of every row hits[q][: n_hits[q]] -> int64 [n_q][k_in][n_fields] (SS_NO_FIELD_VALUE for a
        row outside the table; rows past n_hits[q] keep what the array held, zeros here).  out: the caller's array."""
        hits, n_hits, n_q, k_in = self._window(hits, n_hits, k_in)
        n_fields = getattr(self, "n_fields", 0)
        if out is None:
            out = np.zeros((n_q, k_in, n_fields), dtype=np.int64)
        elif (out.numel() * out.element_size() if _is_torch(out) else out.nbytes) < n_q * k_in * n_fields * 8:
            raise ValueError("output buffer too small")
        self.ctx.ready(hits, n_hits, out)
        check(self.ctx.lib.ss_hit_fields(self.h, n_q, k_in, _ptr(hits), _ptr(n_hits), _ptr(out)), self.ctx.h)
        if _is_torch(out) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()
        return out

    def set_doc_vectors(self, vec) -> None:
        """ss_scorer_set_doc_vectors: register one int8 vector per doc (int8 [n_docs][dim] doc-major, numpy or torch, dim a multiple of
        64 up to SS_MAX_VEC_DIM), or None to clear.  Replaces the previous table once the scorer's outstanding work is done."""
        if vec is None:
            check(self.ctx.lib.ss_scorer_set_doc_vectors(self.h, 0, None), self.ctx.h)
            self.vec_dim = 0
            self.n_vec_lists = 0
            return
        vec = _as(vec, "int8")
        if vec.ndim != 2 or int(vec.shape[0]) != self.title.n_docs:
            raise ValueError(f"vector table must have shape [{self.title.n_docs}][dim], got {tuple(vec.shape)}")
        self.ctx.ready(vec)
        check(self.ctx.lib.ss_scorer_set_doc_vectors(self.h, int(vec.shape[1]), _ptr(vec)), self.ctx.h)
        self.vec_dim = int(vec.shape[1])
        self.n_vec_lists = 0                        # (the library drops the lists: they describe the old table)

    def _qvec(self, qvec):
        qvec = _as(qvec, "int8")
        if qvec.ndim != 2 or (getattr(self, "vec_dim", 0) and int(qvec.shape[1]) != self.vec_dim):
            raise ValueError(f"query vectors must have shape [n_q][{getattr(self, 'vec_dim', 0)}], got {tuple(qvec.shape)}")
        return qvec, int(qvec.shape[0])

    def vector_topk(self, qvec, k: int, mask_id=None, device_out: bool = False, out=None):
        """ss_vector_topk: per query vector the exact k nearest docs by integer dot product over the table of set_doc_vectors (score
        descending, doc ascending), restricted to the registered allow-list mask_id[q] (-1 / None: every doc) ->
        (hits VEC_HIT_DTYPE [n_q][k], n_hits int32 [n_q]).  device_out: torch device tensors (hits as int32 [n_q][k][2]: doc bits,
        score); out = (hits, n_hits): the caller's arrays, returned as they are.  With device arrays throughout the library only
        enqueues."""
        qvec, n_q = self._qvec(qvec)
        mask_id = _as(mask_id, "int32")
        if out is None:
            if device_out:
                import torch
                dev = qvec.device if _is_torch(qvec) and qvec.is_cuda else torch.device("cuda", self.ctx.device_id)
                out = (torch.zeros((n_q, int(k), 2), dtype=torch.int32, device=dev), torch.zeros(n_q, dtype=torch.int32, device=dev))
            else:
                out = (np.zeros((n_q, int(k)), dtype=VEC_HIT_DTYPE), np.zeros(n_q, dtype=np.int32))
        hits, n_hits = out
        n_hits = _as(n_hits, "int32")
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        if int(k) > 0 and (nbytes(hits) < n_q * int(k) * 8 or nbytes(n_hits) < n_q * 4):
            raise ValueError("output buffers too small")
        self.ctx.ready(qvec, mask_id, hits, n_hits)
        check(self.ctx.lib.ss_vector_topk(self.h, n_q, _ptr(qvec), _ptr(mask_id), int(k), _ptr(hits), _ptr(n_hits)), self.ctx.h)
        if _is_torch(hits) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return hits, n_hits

    def set_vector_lists(self, centroids, list_of_doc) -> None:
        """ss_scorer_set_vector_lists: register a partition of the vector table: centroids int8 [n_lists][dim] and list_of_doc uint32
        [n_docs] (every entry below n_lists, or NO_LIST for a doc no probed search finds), numpy or torch; None clears.  Needs
        set_doc_vectors, which also drops the lists.  Keeps a second, list-major copy of the table on the device."""
        if centroids is None:
            check(self.ctx.lib.ss_scorer_set_vector_lists(self.h, 0, None, None), self.ctx.h)
            self.n_vec_lists = 0
            return
        centroids, list_of_doc = _as(centroids, "int8"), _as(list_of_doc, "uint32")
        if centroids.ndim != 2 or (getattr(self, "vec_dim", 0) and int(centroids.shape[1]) != self.vec_dim):
            raise ValueError(f"centroids must have shape [n_lists][{getattr(self, 'vec_dim', 0)}], got {tuple(centroids.shape)}")
        if list_of_doc.ndim != 1 or int(list_of_doc.shape[0]) != self.title.n_docs:
            raise ValueError(f"list_of_doc must have shape [{self.title.n_docs}], got {tuple(list_of_doc.shape)}")
        self.ctx.ready(centroids, list_of_doc)
        check(self.ctx.lib.ss_scorer_set_vector_lists(self.h, int(centroids.shape[0]), _ptr(centroids), _ptr(list_of_doc)), self.ctx.h)
        self.n_vec_lists = int(centroids.shape[0])

    def assign_vector_lists(self, centroids, device_out: bool = False, out=None, want_scores: bool = True):
        """ss_vector_assign_lists: per doc of the vector table the list of the centroid (int8 [n_lists][dim]) with the largest integer
        dot product, ties to the lower list -> (list_of_doc uint32 [n_docs], scores int32 [n_docs] | None).  Registers nothing.
        device_out: torch device tensors (the lists as int32 bits); out = (lists, scores | None): the caller's arrays."""
        centroids = _as(centroids, "int8")
        if centroids.ndim != 2 or (getattr(self, "vec_dim", 0) and int(centroids.shape[1]) != self.vec_dim):
            raise ValueError(f"centroids must have shape [n_lists][{getattr(self, 'vec_dim', 0)}], got {tuple(centroids.shape)}")
        n = self.title.n_docs
        if out is None:
            if device_out:
                import torch
                dev = torch.device("cuda", self.ctx.device_id)
                out = (torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev) if want_scores else None)
            else:
                out = (np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32) if want_scores else None)
        lists, scores = out
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        if nbytes(lists) < n * 4 or (scores is not None and nbytes(scores) < n * 4):
            raise ValueError("output buffers too small")
        self.ctx.ready(centroids, lists, scores)
        check(self.ctx.lib.ss_vector_assign_lists(self.h, int(centroids.shape[0]), _ptr(centroids), _ptr(lists), _ptr(scores)), self.ctx.h)
        if _is_torch(lists) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()
        return lists, scores

    def vector_topk_probed(self, qvec, k: int, n_probe: int, mask_id=None, device_out: bool = False, out=None, return_probes: bool = False):
        """ss_vector_topk_probed: vector_topk over the docs of the min(n_probe, n_lists) lists of set_vector_lists whose centroids score
        highest under the query (score descending, list ascending): exact within them, and vector_topk's bytes when every list is
        probed and no doc is at NO_LIST -> (hits, n_hits), with return_probes (hits, n_hits, probes uint32 [n_q][min(n_probe,
        n_lists)]).  device_out / out = (hits, n_hits[, probes]) as in vector_topk."""
        qvec, n_q = self._qvec(qvec)
        mask_id = _as(mask_id, "int32")
        n_p = max(1, min(int(n_probe), getattr(self, "n_vec_lists", 0) or int(n_probe)))
        if out is None:
            if device_out:
                import torch
                dev = qvec.device if _is_torch(qvec) and qvec.is_cuda else torch.device("cuda", self.ctx.device_id)
                out = (torch.zeros((n_q, int(k), 2), dtype=torch.int32, device=dev), torch.zeros(n_q, dtype=torch.int32, device=dev),
                       torch.zeros((n_q, n_p), dtype=torch.int32, device=dev) if return_probes else None)
            else:
                out = (np.zeros((n_q, int(k)), dtype=VEC_HIT_DTYPE), np.zeros(n_q, dtype=np.int32),
                       np.zeros((n_q, n_p), dtype=np.uint32) if return_probes else None)
        hits, n_hits = out[0], _as(out[1], "int32")
        probes = out[2] if len(out) > 2 else None
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        if int(k) > 0 and (nbytes(hits) < n_q * int(k) * 8 or nbytes(n_hits) < n_q * 4 or (probes is not None and nbytes(probes) < n_q * n_p * 4)):
            raise ValueError("output buffers too small")
        self.ctx.ready(qvec, mask_id, hits, n_hits, probes)
        check(self.ctx.lib.ss_vector_topk_probed(self.h, n_q, _ptr(qvec), _ptr(mask_id), int(k), int(n_probe), _ptr(hits), _ptr(n_hits),
                                                 _ptr(probes)), self.ctx.h)
        if _is_torch(hits) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return (hits, n_hits, probes) if return_probes or len(out) > 2 and probes is not None else (hits, n_hits)

    def hit_vector_scores(self, qvec, hits, n_hits, k_in: Optional[int] = None, out=None):
        """ss_hit_vector_scores: the score of every row hits[q][: n_hits[q]] under query vector q -> int32 [n_q][k_in]
        (SS_NO_VEC_SCORE for a row outside the table; rows past n_hits[q] keep what the array held, zeros here).  out: the caller's
        array."""
        qvec, _ = self._qvec(qvec)
        hits, n_hits, n_q, k_in = self._window(hits, n_hits, k_in)
        if out is None:
            out = np.zeros((n_q, k_in), dtype=np.int32)
        elif (out.numel() * out.element_size() if _is_torch(out) else out.nbytes) < n_q * k_in * 4:
            raise ValueError("output buffer too small")
        self.ctx.ready(qvec, hits, n_hits, out)
        check(self.ctx.lib.ss_hit_vector_scores(self.h, n_q, _ptr(qvec), k_in, _ptr(hits), _ptr(n_hits), _ptr(out)), self.ctx.h)
        if _is_torch(out) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()
        return out

    def rerank_hits_by_vector(self, qvec, hits, n_hits, k: int, first: int = 0, k_in: Optional[int] = None, out=None,
                              want_scores: bool = True):
        """ss_rerank_hits_by_vector: every window hits[q][: n_hits[q]] sorted stably by its score under query vector q, descending
        (rows outside the table last), page [first, first + k) -> (hits [n_q][k], n_hits [n_q], scores [n_q][k] int32 | None).
        hits / n_hits, k_in as in collapse_hits.  out = (hits, n_hits, scores | None): the caller's arrays, returned as they are;
        with device arrays throughout the library only enqueues."""
        qvec, _ = self._qvec(qvec)
        hits, n_hits, n_q, k_in = self._window(hits, n_hits, k_in)
        if out is None:
            out = (np.zeros((n_q, int(k)), dtype=HIT_DTYPE), np.zeros(n_q, dtype=np.int32),
                   np.zeros((n_q, int(k)), dtype=np.int32) if want_scores else None)
        o_hits, o_n, o_sc = out
        o_n, o_sc = _as(o_n, "int32"), _as(o_sc, "int32")
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        if int(k) > 0 and (nbytes(o_hits) < n_q * int(k) * HIT_DTYPE.itemsize or nbytes(o_n) < n_q * 4
                           or (o_sc is not None and nbytes(o_sc) < n_q * int(k) * 4)):
            raise ValueError("output buffers too small")
        self.ctx.ready(qvec, hits, n_hits, o_hits, o_n, o_sc)
        check(self.ctx.lib.ss_rerank_hits_by_vector(self.h, n_q, _ptr(qvec), k_in, _ptr(hits), _ptr(n_hits), int(first), int(k),
                                                    _ptr(o_hits), _ptr(o_n), _ptr(o_sc)), self.ctx.h)
        if _is_torch(o_hits) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return o_hits, o_n, o_sc

    def set_doc_tokens(self, tok_ptr, tok) -> None:
        """ss_scorer_set_doc_tokens: register the token vectors of every doc: tok_ptr uint64 [n_docs + 1] (torch: int64 of the same
        bits), tok int8 [tok_ptr[n_docs]][dim] (numpy or torch, dim a multiple of 64 up to SS_MAX_VEC_DIM), doc d's tokens at rows
        tok_ptr[d] .. tok_ptr[d + 1]; tok None clears.  Independent of set_doc_vectors.  Replaces the previous table once the scorer's
        outstanding work is done."""
        if tok is None:
            check(self.ctx.lib.ss_scorer_set_doc_tokens(self.h, 0, None, None), self.ctx.h)
            self.tok_dim = 0
            return
        tok_ptr, tok = _as(tok_ptr, "uint64"), _as(tok, "int8")
        n_ptr = int(tok_ptr.numel() if _is_torch(tok_ptr) else tok_ptr.size)
        if n_ptr != self.title.n_docs + 1:
            raise ValueError(f"tok_ptr must have {self.title.n_docs + 1} entries, got {n_ptr}")
        if tok.ndim != 2 or int(tok.shape[0]) < int(tok_ptr[-1]):
            raise ValueError(f"token table must have shape [tok_ptr[n_docs] = {int(tok_ptr[-1])}][dim], got {tuple(tok.shape)}")
        self.ctx.ready(tok_ptr, tok)
        check(self.ctx.lib.ss_scorer_set_doc_tokens(self.h, int(tok.shape[1]), _ptr(tok_ptr), _ptr(tok)), self.ctx.h)
        self.tok_dim = int(tok.shape[1])

    def _qtok(self, qt_ptr, qtok, n_q: int):
        """(qt_ptr, qtok) of a MaxSim call: qt_ptr uint32 [n_q + 1], qtok int8 [qt_ptr[n_q]][dim] (None: no query has a token)"""
        qt_ptr, qtok = _as(qt_ptr, "uint32"), _as(qtok, "int8")
        n_ptr = int(qt_ptr.numel() if _is_torch(qt_ptr) else qt_ptr.size)
        if n_ptr != n_q + 1:
            raise ValueError(f"qt_ptr must have n_q + 1 = {n_q + 1} entries, got {n_ptr}")
        if qtok is not None:
            dim = getattr(self, "tok_dim", 0)
            if qtok.ndim != 2 or (dim and int(qtok.shape[1]) != dim) or int(qtok.shape[0]) < int(qt_ptr[-1]):
                raise ValueError(f"query tokens must have shape [qt_ptr[n_q] = {int(qt_ptr[-1])}][{dim}], got {tuple(qtok.shape)}")
        return qt_ptr, qtok

    def hit_maxsim_scores(self, qt_ptr, qtok, hits, n_hits, k_in: Optional[int] = None, out=None):
        """ss_hit_maxsim_scores: the late-interaction score of every row hits[q][: n_hits[q]] under the token vectors of query q (the
        sum over the query's tokens of the best dot product among the doc's tokens) -> int32 [n_q][k_in] (SS_NO_VEC_SCORE for a row
        outside the table or a doc without tokens; rows past n_hits[q] keep what the array held, zeros here).  qt_ptr uint32
        [n_q + 1], read on the host; qtok int8 [qt_ptr[n_q]][dim].  out: the caller's array."""
        hits, n_hits, n_q, k_in = self._window(hits, n_hits, k_in)
        qt_ptr, qtok = self._qtok(qt_ptr, qtok, n_q)
        if out is None:
            out = np.zeros((n_q, k_in), dtype=np.int32)
        elif (out.numel() * out.element_size() if _is_torch(out) else out.nbytes) < n_q * k_in * 4:
            raise ValueError("output buffer too small")
        self.ctx.ready(qt_ptr, qtok, hits, n_hits, out)
        check(self.ctx.lib.ss_hit_maxsim_scores(self.h, n_q, _ptr(qt_ptr), _ptr(qtok), k_in, _ptr(hits), _ptr(n_hits), _ptr(out)), self.ctx.h)
        if _is_torch(out) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()
        return out

    def rerank_hits_by_maxsim(self, qt_ptr, qtok, hits, n_hits, k: int, first: int = 0, k_in: Optional[int] = None, out=None,
                              want_scores: bool = True):
        """ss_rerank_hits_by_maxsim: every window hits[q][: n_hits[q]] sorted stably by its late-interaction score under the token
        vectors of query q, descending (rows without a score last), page [first, first + k) -> (hits [n_q][k], n_hits [n_q], scores
        [n_q][k] int32 | None).  qt_ptr / qtok as in hit_maxsim_scores; hits / n_hits, k_in as in collapse_hits.  out = (hits, n_hits,
        scores | None): the caller's arrays, returned as they are; with device arrays throughout the library only enqueues."""
        hits, n_hits, n_q, k_in = self._window(hits, n_hits, k_in)
        qt_ptr, qtok = self._qtok(qt_ptr, qtok, n_q)
        if out is None:
            out = (np.zeros((n_q, int(k)), dtype=HIT_DTYPE), np.zeros(n_q, dtype=np.int32),
                   np.zeros((n_q, int(k)), dtype=np.int32) if want_scores else None)
        o_hits, o_n, o_sc = out
        o_n, o_sc = _as(o_n, "int32"), _as(o_sc, "int32")
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        if int(k) > 0 and (nbytes(o_hits) < n_q * int(k) * HIT_DTYPE.itemsize or nbytes(o_n) < n_q * 4
                           or (o_sc is not None and nbytes(o_sc) < n_q * int(k) * 4)):
            raise ValueError("output buffers too small")
        self.ctx.ready(qt_ptr, qtok, hits, n_hits, o_hits, o_n, o_sc)
        check(self.ctx.lib.ss_rerank_hits_by_maxsim(self.h, n_q, _ptr(qt_ptr), _ptr(qtok), k_in, _ptr(hits), _ptr(n_hits), int(first), int(k),
                                                    _ptr(o_hits), _ptr(o_n), _ptr(o_sc)), self.ctx.h)
        if _is_torch(o_hits) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return o_hits, o_n, o_sc

    def maxsim_topk(self, qt_ptr, qtok, k: int, mask_id=None, device_out: bool = False, out=None):
        """ss_maxsim_topk: per query the exact k best docs by late-interaction score over every doc of set_doc_tokens that has a
        token (score descending, doc ascending), restricted to the registered allow-list mask_id[q] (-1 / None: every doc) ->
        (hits VEC_HIT_DTYPE [n_q][k], n_hits int32 [n_q]).  qt_ptr uint32 [n_q + 1], read on the host; qtok int8 [qt_ptr[n_q]][dim]
        (None: no query has a token).  device_out: torch device tensors (hits as int32 [n_q][k][2]: doc bits, score); out = (hits,
        n_hits): the caller's arrays, returned as they are.  With device arrays throughout the library only enqueues."""
        qt_ptr = _as(qt_ptr, "uint32")
        n_q = int(qt_ptr.numel() if _is_torch(qt_ptr) else qt_ptr.size) - 1
        if n_q < 0:
            raise ValueError("qt_ptr must have n_q + 1 entries")
        qt_ptr, qtok = self._qtok(qt_ptr, qtok, n_q)
        mask_id = _as(mask_id, "int32")
        if out is None:
            if device_out:
                import torch
                dev = qtok.device if _is_torch(qtok) and qtok.is_cuda else torch.device("cuda", self.ctx.device_id)
                out = (torch.zeros((n_q, int(k), 2), dtype=torch.int32, device=dev), torch.zeros(n_q, dtype=torch.int32, device=dev))
            else:
                out = (np.zeros((n_q, int(k)), dtype=VEC_HIT_DTYPE), np.zeros(n_q, dtype=np.int32))
        hits, n_hits = out
        n_hits = _as(n_hits, "int32")
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        if int(k) > 0 and (nbytes(hits) < n_q * int(k) * 8 or nbytes(n_hits) < n_q * 4):
            raise ValueError("output buffers too small")
        self.ctx.ready(qt_ptr, qtok, mask_id, hits, n_hits)
        check(self.ctx.lib.ss_maxsim_topk(self.h, n_q, _ptr(qt_ptr), _ptr(qtok), _ptr(mask_id), int(k), _ptr(hits), _ptr(n_hits)), self.ctx.h)
        if _is_torch(hits) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return hits, n_hits

    def diversify_hits(self, qvec, hits, n_hits, k: int, w_rel: int, w_div: int, first: int = 0, k_in: Optional[int] = None, out=None,
                       want_info: bool = True):
        """ss_diversify_hits: every window hits[q][: n_hits[q]] re-ranked greedily, each next row the one with the largest
        w_rel * rel - w_div * (largest similarity to a row already chosen), ties to the earlier row; rows outside the table last; page
        [first, first + k) -> (hits [n_q][k], n_hits [n_q], info [n_q][k] DIV_INFO_DTYPE | None).  qvec: int8 [n_q][dim], rel = the
        row's score under it, or None: rel = minus the window position.  w_rel, w_div: integers in [0, SS_DIV_WEIGHT_MAX].  hits /
        n_hits, k_in as in collapse_hits.  out = (hits, n_hits, info | None): the caller's arrays, returned as they are; with device
        arrays throughout the library only enqueues."""
        if qvec is not None:
            qvec, _ = self._qvec(qvec)
        hits, n_hits, n_q, k_in = self._window(hits, n_hits, k_in)
        if qvec is not None and int(qvec.shape[0]) != n_q:
            raise ValueError(f"{int(qvec.shape[0])} query vectors for {n_q} windows")
        if out is None:
            out = (np.zeros((n_q, int(k)), dtype=HIT_DTYPE), np.zeros(n_q, dtype=np.int32),
                   np.zeros((n_q, int(k)), dtype=DIV_INFO_DTYPE) if want_info else None)
        o_hits, o_n, o_info = out
        o_n = _as(o_n, "int32")
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        if int(k) > 0 and (nbytes(o_hits) < n_q * int(k) * HIT_DTYPE.itemsize or nbytes(o_n) < n_q * 4
                           or (o_info is not None and nbytes(o_info) < n_q * int(k) * DIV_INFO_DTYPE.itemsize)):
            raise ValueError("output buffers too small")
        self.ctx.ready(qvec, hits, n_hits, o_hits, o_n, o_info)
        check(self.ctx.lib.ss_diversify_hits(self.h, n_q, _ptr(qvec), k_in, _ptr(hits), _ptr(n_hits), int(w_rel), int(w_div), int(first),
                                             int(k), _ptr(o_hits), _ptr(o_n), _ptr(o_info)), self.ctx.h)
        if _is_torch(o_hits) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return o_hits, o_n, o_info

    @staticmethod
    def _fuse_params(mode: int, rrf_c: int, w_lex: float, w_vec: float):
        from ._lib import SsFuseParams
        return SsFuseParams(int(mode), int(rrf_c), float(w_lex), float(w_vec))

    def _fuse_out(self, n_q: int, k: int, out, want_fused: bool, want_union: bool, like=None):
        """(hits, n_hits, fused | None, n_union | None): the caller's arrays, or fresh numpy ones"""
        if out is None:
            out = (np.zeros((n_q, k), dtype=HIT_DTYPE), np.zeros(n_q, dtype=np.int32),
                   np.zeros((n_q, k), dtype=FUSED_DTYPE) if want_fused else None, np.zeros(n_q, dtype=np.int32) if want_union else None)
        o_hits, o_n, o_fused, o_union = out
        o_n, o_union = _as(o_n, "int32"), _as(o_union, "int32")
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        if k > 0 and (nbytes(o_hits) < n_q * k * HIT_DTYPE.itemsize or nbytes(o_n) < n_q * 4
                      or (o_fused is not None and nbytes(o_fused) < n_q * k * FUSED_DTYPE.itemsize)
                      or (o_union is not None and nbytes(o_union) < n_q * 4)):
            raise ValueError("output buffers too small")
        return o_hits, o_n, o_fused, o_union

    def score_docs(self, q_ptr, q_terms, docs, n_in=None, query_len=None, topic_probs=None, out=None):
        """ss_score_docs: the row that query q's ranking holds for every doc docs[q][: n_in[q]], whether or not it would reach any
        top-k -> hits HIT_DTYPE [n_q][k_in] (a doc outside the table: a zero row with its id; rows past n_in[q] keep what the array
        held, zeros here).  docs uint32 [n_q][k_in] and n_in int32 [n_q] (None: all k_in), numpy or torch; out: the caller's array.
        With docs, n_in and out on the device the library only enqueues."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        query_len = _as(query_len, "int32")
        topic_probs = _as(topic_probs, "float64")
        docs = _as(docs, "uint32")
        n_q = int(q_ptr.shape[0]) - 1
        if docs.ndim != 2 or int(docs.shape[0]) != n_q:
            raise ValueError(f"docs must have shape [{n_q}][k_in], got {tuple(docs.shape)}")
        k_in = int(docs.shape[1])
        if n_in is None:
            n_in = np.full(n_q, k_in, dtype=np.int32)
        n_in = _as(n_in, "int32")
        if out is None:
            out = np.zeros((n_q, k_in), dtype=HIT_DTYPE)
        elif (out.numel() * out.element_size() if _is_torch(out) else out.nbytes) < n_q * k_in * HIT_DTYPE.itemsize:
            raise ValueError("output buffer too small")
        self.ctx.ready(q_ptr, q_terms, query_len, topic_probs, docs, n_in, out)
        check(self.ctx.lib.ss_score_docs(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(query_len), _ptr(topic_probs), k_in, _ptr(docs),
                                         _ptr(n_in), _ptr(out)), self.ctx.h)
        if _is_torch(out) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()
        return out

    def fuse_hits(self, q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, k: int, mode: int = FUSE_RRF, rrf_c: int = 60, w_lex: float = 1.0,
                  w_vec: float = 1.0, first: int = 0, k_lex: Optional[int] = None, k_vec: Optional[int] = None, query_len=None,
                  topic_probs=None, out=None, want_fused: bool = True, want_union: bool = True):
        """ss_fuse_hits: the lexical list lex[q][: n_lex[q]] (rows of any scoring call) and the vector list vec[q][: n_vec[q]]
        (VEC_HIT_DTYPE rows of vector_topk, or the torch int32 [n_q][k][2] tensors it returns) fused per query by reciprocal rank
        (FUSE_RRF: w_lex / (rrf_c + lex_rank) + w_vec / (rrf_c + vec_rank)) or by FUSE_WEIGHTED: w_lex * final + w_vec * vec_score;
        a doc only one list holds is completed by score_docs / hit_vector_scores.  Page [first, first + k) of score descending, doc
        ascending -> (hits [n_q][k], n_hits [n_q], fused FUSED_DTYPE [n_q][k] | None, n_union [n_q] | None).  out = the caller's four
        arrays, returned as they are; with device arrays throughout the library only enqueues."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        query_len = _as(query_len, "int32")
        topic_probs = _as(topic_probs, "float64")
        qvec, _ = self._qvec(qvec)
        lex, n_lex, n_q, k_lex = self._window(lex, n_lex, k_lex)
        n_vec = _as(n_vec, "int32")
        nbytes = lambda a: a.numel() * a.element_size() if _is_torch(a) else a.nbytes      # noqa: E731
        vec = vec.contiguous() if _is_torch(vec) else np.ascontiguousarray(vec, dtype=VEC_HIT_DTYPE)
        if k_vec is None:
            k_vec = nbytes(vec) // (n_q * VEC_HIT_DTYPE.itemsize) if n_q > 0 else 1
        elif nbytes(vec) < n_q * int(k_vec) * VEC_HIT_DTYPE.itemsize:
            raise ValueError("vec too small")
        o_hits, o_n, o_fused, o_union = self._fuse_out(n_q, int(k), out, want_fused, want_union)
        fp = self._fuse_params(mode, rrf_c, w_lex, w_vec)
        self.ctx.ready(q_ptr, q_terms, query_len, topic_probs, qvec, lex, n_lex, vec, n_vec, o_hits, o_n, o_fused, o_union)
        check(self.ctx.lib.ss_fuse_hits(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(query_len), _ptr(topic_probs), _ptr(qvec),
                                        int(k_lex), _ptr(lex), _ptr(n_lex), int(k_vec), _ptr(vec), _ptr(n_vec), C.byref(fp), int(first),
                                        int(k), _ptr(o_hits), _ptr(o_n), _ptr(o_fused), _ptr(o_union)), self.ctx.h)
        if _is_torch(o_hits) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return o_hits, o_n, o_fused, o_union

    def hybrid_topk(self, q_ptr, q_terms, qvec, k_window: int, k: int, mode: int = FUSE_RRF, rrf_c: int = 60, w_lex: float = 1.0,
                    w_vec: float = 1.0, first: int = 0, mask_id=None, query_len=None, topic_probs=None, out=None,
                    want_fused: bool = True, want_union: bool = True):
        """ss_hybrid_topk: fuse_hits applied to the rows score_topk_masked and vector_topk give at k = k_window under mask_id, without
        either window leaving the device -> (hits [n_q][k], n_hits [n_q], fused | None, n_union | None).  out as in fuse_hits: with
        device arrays the library only enqueues."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        query_len = _as(query_len, "int32")
        topic_probs = _as(topic_probs, "float64")
        mask_id = _as(mask_id, "int32")
        qvec, _ = self._qvec(qvec)
        n_q = int(q_ptr.shape[0]) - 1
        o_hits, o_n, o_fused, o_union = self._fuse_out(n_q, int(k), out, want_fused, want_union)
        fp = self._fuse_params(mode, rrf_c, w_lex, w_vec)
        self.ctx.ready(q_ptr, q_terms, query_len, topic_probs, qvec, mask_id, o_hits, o_n, o_fused, o_union)
        check(self.ctx.lib.ss_hybrid_topk(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(query_len), _ptr(topic_probs), _ptr(qvec),
                                          _ptr(mask_id), int(k_window), C.byref(fp), int(first), int(k), _ptr(o_hits), _ptr(o_n),
                                          _ptr(o_fused), _ptr(o_union)), self.ctx.h)
        if _is_torch(o_hits) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return o_hits, o_n, o_fused, o_union

    def submit(self, q_ptr, q_terms, k: int, query_len=None, topic_probs=None, p_ptr=None, p_terms=None):
        """ss_score_topk_submit: enqueue a batch whose hits go to host memory; -> ticket for collect().
        p_ptr / p_terms: the queries' quoted phrases as in score_topk_phrase (None: plain OR queries)."""
        q_ptr = _as(q_ptr, "uint32")
        q_terms = _as(q_terms, "uint32")
        p_ptr = _as(p_ptr, "uint32")
        p_terms = _as(p_terms, "uint32")
        query_len = _as(query_len, "int32")
        topic_probs = _as(topic_probs, "float64")
        n_q = int(q_ptr.shape[0]) - 1
        self.ctx.ready(q_ptr, q_terms, p_ptr, p_terms, query_len, topic_probs)
        ticket = C.c_uint64(0)
        check(self.ctx.lib.ss_score_topk_submit(self.h, n_q, _ptr(q_ptr), _ptr(q_terms), _ptr(p_ptr), _ptr(p_terms), _ptr(query_len),
                                                _ptr(topic_probs), k, C.addressof(ticket)), self.ctx.h)
        return (int(ticket.value), n_q, k)

    def collect(self, ticket, out=None):
        """ss_score_topk_collect: wait for the batch of `ticket` (from submit) -> (hits [n_q][k], n_hits [n_q]) in host memory."""
        t, n_q, k = ticket
        hits, n_hits = out if out is not None else (np.zeros((n_q, k), dtype=HIT_DTYPE), np.zeros(n_q, dtype=np.int32))
        check(self.ctx.lib.ss_score_topk_collect(self.h, t, hits.ctypes.data, n_hits.ctypes.data), self.ctx.h)
        return hits, n_hits

    def close(self) -> None:
        if self.h:
            self.ctx.lib.ss_scorer_destroy(self.h)
            self.h = None

NO_LIST = 0xFFFFFFFF             # SS_NO_LIST


def train_vector_lists(scorer: "Scorer", vec, n_lists: int, iters: int = 5, seed: int = 0):
    """A convenience, not part of the ABI: k-means-style centroids for Scorer.set_vector_lists over the table `vec` (int8 [n_docs][dim],
    registered on `scorer` by set_doc_vectors).  Centroids start as n_lists rows of vec drawn without replacement by
    np.random.default_rng(seed); every iteration assigns on the device (assign_vector_lists) and replaces each centroid by
    np.rint of the float64 mean of its docs, clipped to int8; an empty list keeps its centroid.  Returns (centroids int8
    [n_lists][dim], list_of_doc uint32 [n_docs]) with list_of_doc the assignment to the centroids returned.  Defined as what
    tests/vector_lists_model.py: train does."""
    vec = np.ascontiguousarray(vec, dtype=np.int8)
    n_docs = vec.shape[0]
    rng = np.random.default_rng(seed)
    centroids = vec[np.sort(rng.choice(n_docs, size=int(n_lists), replace=False))].copy()
    for _ in range(int(iters)):
        lists, _scores = scorer.assign_vector_lists(centroids, want_scores=False)
        sums = np.zeros((int(n_lists), vec.shape[1]), np.float64)
        np.add.at(sums, lists, vec.astype(np.float64))
        cnt = np.bincount(lists, minlength=int(n_lists))
        live = cnt > 0
        centroids[live] = np.clip(np.rint(sums[live] / cnt[live, None]), -128, 127).astype(np.int8)
    lists, _scores = scorer.assign_vector_lists(centroids, want_scores=False)
    return centroids, lists


__all__ = ["Context", "Graph", "PageRankState", "InvertedIndex", "Scorer", "HIT_DTYPE", "TERM_MATCH_DTYPE", "PASSAGE_DTYPE", "PROXIMITY_DTYPE", "SsHit", "SsTermMatch", "SsPassage", "SsProximity",
           "pack_doc_masks", "DOC_RANGE_DTYPE", "pack_doc_ranges", "VEC_HIT_DTYPE", "FUSED_DTYPE", "FUSE_RRF", "FUSE_WEIGHTED", "NO_LIST", "train_vector_lists",
           "TREE_NODE_DTYPE", "RANK_N_FEATURES", "RankModel"]


def _flatten_words(words, ptr_dtype: str):
    """A sequence of words (bytes, or str encoded as UTF-8) -> (ptr [n + 1], bytes uint8); a (ptr, bytes) pair of arrays (numpy or
    torch: int64 / int32 ptr, uint8 bytes) passes through."""
    if isinstance(words, tuple) and len(words) == 2 and not isinstance(words[0], (bytes, str)):
        return _as(words[0], ptr_dtype), _as(words[1], "uint8")
    raw = [w.encode("utf-8") if isinstance(w, str) else bytes(w) for w in words]
    ptr = np.zeros(len(raw) + 1, dtype=np.dtype(ptr_dtype))
    if raw:
        total = np.cumsum([len(w) for w in raw], dtype=np.uint64)
        if ptr_dtype == "uint32" and int(total[-1]) >= 1 << 32:
            raise ValueError("2^32 bytes of words or more in one call")
        ptr[1:] = total
    return ptr, np.frombuffer(b"".join(raw), dtype=np.uint8).copy()


class Lexicon:
    """ss_lexicon: the vocabulary's words on the device, keyed by term id: the word list by prefix and spelling suggestions.
    words: a sequence of bytes / str (word t = words[t]) or a (word_ptr uint64 [n + 1], bytes uint8) pair; freq uint32 [n] or None
    (all 0).  Immutable apart from freq: after an index update that adds terms, close it and make a new one."""

    def __init__(self, ctx: Context, words, freq=None):
        self.ctx = ctx
        ptr, data = _flatten_words(words, "uint64")
        self.n_terms = int(ptr.shape[0]) - 1
        freq = _as(freq, "uint32")
        if freq is not None and (freq.numel() if _is_torch(freq) else freq.size) != self.n_terms:
            raise ValueError("freq must hold one value per word")
        ctx.ready(ptr, data, freq)
        h = C.c_void_p()
        check(ctx.lib.ss_lexicon_create(ctx.h, self.n_terms, _ptr(ptr), _ptr(data), _ptr(freq), C.byref(h)), ctx.h)
        self.h = h

    def close(self) -> None:
        if self.h:
            check(self.ctx.lib.ss_lexicon_destroy(self.h), self.ctx.h)
            self.h = None

    def info(self):
        """-> (n_terms, n_bytes)"""
        n, b = C.c_uint64(), C.c_uint64()
        check(self.ctx.lib.ss_lexicon_get_info(self.h, C.byref(n), C.byref(b)), self.ctx.h)
        return n.value, b.value

    def set_freq(self, freq) -> None:
        """ss_lexicon_set_freq: replace the popularity of every word (uint32 [n_terms], numpy or torch; None = all 0)."""
        freq = _as(freq, "uint32")
        if freq is not None and (freq.numel() if _is_torch(freq) else freq.size) != self.n_terms:
            raise ValueError("freq must hold one value per word")
        self.ctx.ready(freq)
        check(self.ctx.lib.ss_lexicon_set_freq(self.h, _ptr(freq)), self.ctx.h)

    def order(self, out=None):
        """ss_lexicon_read_order: the permutation that sorts the words (unsigned bytes, a proper prefix first, equal words by id)."""
        if out is None:
            out = np.zeros(self.n_terms, dtype=np.uint32)
        else:
            out = _as(out, "uint32")
            if (out.numel() if _is_torch(out) else out.size) < self.n_terms:
                raise ValueError("output buffer too small")
        self.ctx.ready(out)
        check(self.ctx.lib.ss_lexicon_read_order(self.h, _ptr(out)), self.ctx.h)
        return out

    def prefix(self, prefixes, k: int, first: int = 0, out=None):
        """ss_lexicon_prefix: per prefix the page [first, first + k) of the terms whose word starts with it, in sort order
        -> (terms uint32 [n_q][k], n_out int32 [n_q], n_match uint64 [n_q]); entries past n_out[q] keep what the array held (zeros
        here).  out = (terms, n_out, n_match | None): the caller's arrays (numpy, or torch int32 / int32 / int64 device tensors); with
        device tensors the library only enqueues."""
        p_ptr, p_bytes = _flatten_words(prefixes, "uint32")
        n_q = int(p_ptr.shape[0]) - 1
        count = lambda a: a.numel() if _is_torch(a) else a.size       # noqa: E731
        if out is not None:
            terms, n_out, n_match = _as(out[0], "uint32"), _as(out[1], "int32"), _as(out[2], "uint64")
            if count(terms) < n_q * k or count(n_out) < n_q or (n_match is not None and count(n_match) < n_q):
                raise ValueError("output buffers too small")
        else:
            terms = np.zeros((n_q, max(int(k), 0)), dtype=np.uint32)
            n_out = np.zeros(n_q, dtype=np.int32)
            n_match = np.zeros(n_q, dtype=np.uint64)
        self.ctx.ready(p_ptr, p_bytes, terms, n_out, n_match)
        check(self.ctx.lib.ss_lexicon_prefix(self.h, n_q, _ptr(p_ptr), _ptr(p_bytes), int(first), int(k), _ptr(terms), _ptr(n_out),
                                             _ptr(n_match)), self.ctx.h)
        if out is not None and _is_torch(terms) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return terms, n_out, n_match

    def complete(self, prefixes, m: int = 10, min_freq: int = 1, out=None):
        """ss_lexicon_complete: per prefix the m most frequent of the words that start with it and whose freq is at least min_freq,
        ordered by freq descending, then by sort position -> (terms uint32 [n_q][m], freq uint32 [n_q][m], n_out int32 [n_q],
        n_match uint64 [n_q]: the words with the prefix, whatever their freq); entries past n_out[q] keep what the arrays held (zeros
        here).  out = (terms, freq | None, n_out, n_match | None): the caller's arrays (numpy, or torch int32 / int32 / int32 / int64
        device tensors); with device tensors the library only enqueues."""
        p_ptr, p_bytes = _flatten_words(prefixes, "uint32")
        n_q = int(p_ptr.shape[0]) - 1
        count = lambda a: a.numel() if _is_torch(a) else a.size       # noqa: E731
        if out is not None:
            terms, freq, n_out, n_match = _as(out[0], "uint32"), _as(out[1], "uint32"), _as(out[2], "int32"), _as(out[3], "uint64")
            if (count(terms) < n_q * m or (freq is not None and count(freq) < n_q * m) or count(n_out) < n_q
                    or (n_match is not None and count(n_match) < n_q)):
                raise ValueError("output buffers too small")
        else:
            terms = np.zeros((n_q, max(int(m), 0)), dtype=np.uint32)
            freq = np.zeros((n_q, max(int(m), 0)), dtype=np.uint32)
            n_out = np.zeros(n_q, dtype=np.int32)
            n_match = np.zeros(n_q, dtype=np.uint64)
        self.ctx.ready(p_ptr, p_bytes, terms, freq, n_out, n_match)
        check(self.ctx.lib.ss_lexicon_complete(self.h, n_q, _ptr(p_ptr), _ptr(p_bytes), int(min_freq), int(m), _ptr(terms), _ptr(freq),
                                               _ptr(n_out), _ptr(n_match)), self.ctx.h)
        if out is not None and _is_torch(terms) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return terms, freq, n_out, n_match

    def suggest(self, words, max_dist: int = 2, m: int = 10, min_freq: int = 1, out=None):
        """ss_lexicon_suggest: per query word the m known words within max_dist edits (optimal string alignment over bytes: insert,
        delete, substitute, swap of adjacent bytes) whose freq is at least min_freq, ordered by distance, then freq descending, then
        term id -> (terms uint32 [n_q][m], dist int32 [n_q][m], n_out int32 [n_q]); entries past n_out[q] keep what the arrays held
        (zeros here).  out = (terms, dist | None, n_out): the caller's arrays (numpy, or torch int32 device tensors); with device
        tensors the library only enqueues."""
        w_ptr, w_bytes = _flatten_words(words, "uint32")
        n_q = int(w_ptr.shape[0]) - 1
        count = lambda a: a.numel() if _is_torch(a) else a.size       # noqa: E731
        if out is not None:
            terms, dist, n_out = _as(out[0], "uint32"), _as(out[1], "int32"), _as(out[2], "int32")
            if count(terms) < n_q * m or (dist is not None and count(dist) < n_q * m) or count(n_out) < n_q:
                raise ValueError("output buffers too small")
        else:
            terms = np.zeros((n_q, max(int(m), 0)), dtype=np.uint32)
            dist = np.zeros((n_q, max(int(m), 0)), dtype=np.int32)
            n_out = np.zeros(n_q, dtype=np.int32)
        self.ctx.ready(w_ptr, w_bytes, terms, dist, n_out)
        check(self.ctx.lib.ss_lexicon_suggest(self.h, n_q, _ptr(w_ptr), _ptr(w_bytes), int(max_dist), int(min_freq), int(m), _ptr(terms),
                                              _ptr(dist), _ptr(n_out)), self.ctx.h)
        if out is not None and _is_torch(terms) and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return terms, dist, n_out


class RankModel:
    """ss_rank_model: a tree ensemble over feature rows (learned ranking), validated by the library when it is made.
    score(x) = base + sum of linear[f] * x[f] over the non-NaN columns + the leaf every tree sends x to, added in tree order.
    trees: a sequence of trees, each a TREE_NODE_DTYPE array (or a sequence of (feature, left, right, nan_left, value) tuples) whose
    node 0 is the root and whose children have larger indices than their parent; or a (tree_ptr uint32 [n_trees + 1], nodes
    TREE_NODE_DTYPE) pair.  linear: float64 [n_features] or None."""

    def __init__(self, ctx: Context, n_features: int, trees, linear=None, base: float = 0.0):
        self.ctx = ctx
        self.h = None
        if isinstance(trees, tuple) and len(trees) == 2 and isinstance(trees[0], np.ndarray) and trees[0].dtype.kind in "ui":
            tree_ptr = np.ascontiguousarray(trees[0], dtype=np.uint32)
            nodes = np.ascontiguousarray(trees[1], dtype=TREE_NODE_DTYPE)
        else:
            parts = [np.asarray(t, dtype=TREE_NODE_DTYPE).reshape(-1) for t in trees]
            tree_ptr = np.zeros(len(parts) + 1, dtype=np.uint32)
            if parts:
                tree_ptr[1:] = np.cumsum([p.size for p in parts])
            nodes = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, dtype=TREE_NODE_DTYPE)
        if linear is not None:
            linear = np.ascontiguousarray(linear, dtype=np.float64)
            if linear.size != int(n_features):
                raise ValueError("linear must hold one weight per feature")
        self.n_features = int(n_features)
        h = C.c_void_p()
        check(ctx.lib.ss_rank_model_create(ctx.h, self.n_features, _ptr(linear), float(base), int(tree_ptr.size) - 1, _ptr(tree_ptr), _ptr(nodes),
                                           C.byref(h)), ctx.h)
        self.h = h

    @staticmethod
    def flatten(tree) -> np.ndarray:
        """A nested tree, {"f", "thr", "nan_left", "l", "r"} (nan_left optional, default False) or {"leaf"}, as a TREE_NODE_DTYPE
        array in pre-order: a node, its whole left subtree, its whole right subtree."""
        rows = []
        stack = [(tree, -1, False)]                 # (node, the row of its parent, whether it is the right child)
        while stack:
            node, parent, is_right = stack.pop()
            me = len(rows)
            if parent >= 0:
                rows[parent][2 if is_right else 1] = me
            if "leaf" in node:
                rows.append([-1, 0, 0, 0, float(node["leaf"])])
            else:
                rows.append([int(node["f"]), 0, 0, int(bool(node.get("nan_left", False))), float(node["thr"])])
                stack.append((node["r"], me, True))
                stack.append((node["l"], me, False))    # (popped first: the left subtree comes right behind its parent)
        out = np.zeros(len(rows), dtype=TREE_NODE_DTYPE)
        for i, r in enumerate(rows):
            out[i] = tuple(r)
        return out

    @classmethod
    def from_nested(cls, ctx: Context, n_features: int, trees, linear=None, base: float = 0.0) -> "RankModel":
        """A model from a list of nested dicts (see flatten)."""
        return cls(ctx, n_features, [cls.flatten(t) for t in trees], linear=linear, base=base)

    def close(self) -> None:
        if self.h:
            check(self.ctx.lib.ss_rank_model_destroy(self.h), self.ctx.h)
            self.h = None

    def info(self) -> dict:
        """ss_rank_model_get_info -> {n_features, n_trees, n_nodes, max_tree_nodes, max_depth}"""
        raw = np.zeros(6, dtype=np.uint32)
        check(self.ctx.lib.ss_rank_model_get_info(self.h, _ptr(raw)), self.ctx.h)
        return {"n_features": int(raw[0]), "n_trees": int(raw[1]), "n_nodes": int(raw[2]), "max_tree_nodes": int(raw[3]), "max_depth": int(raw[4])}

    def eval(self, x, out=None):
        """ss_rank_model_eval: x float64 [n_rows][n_features] (numpy or torch) -> scores float64 [n_rows]; out: the caller's array,
        returned as it is; with x and out in device memory the library only enqueues."""
        x = _as(x, "float64")
        count = lambda a: a.numel() if _is_torch(a) else a.size       # noqa: E731
        if count(x) % self.n_features:
            raise ValueError("x does not hold whole rows of n_features values")
        n_rows = count(x) // self.n_features
        if out is None:
            out = np.zeros(n_rows, dtype=np.float64)
        else:
            out = _as(out, "float64")
            if count(out) < n_rows:
                raise ValueError("output buffer too small")
        self.ctx.ready(x, out)
        check(self.ctx.lib.ss_rank_model_eval(self.h, n_rows, _ptr(x), _ptr(out)), self.ctx.h)
        if _is_torch(out) and out.is_cuda and not getattr(self.ctx, "_shared_stream", False):
            self.ctx.synchronize()                  # (device outputs on the context's own stream: as score_topk)
        return out
