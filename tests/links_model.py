"""Links of a hit (include/spaghetti_rank.h: ss_graph_top_links / ss_graph_hit_links) restated in plain Python / numpy
from (out_ptr, out_dst, key).  The parents come from an explicit transpose of the out-edge CSR; nothing of the library is used."""
import math

import numpy as np

PARENTS, CHILDREN = 0, 1


def edge_lists(n, out_ptr, out_dst, direction):
    """per node the list of its edges' other ends, duplicates kept: children as stored, parents one entry per edge u -> v"""
    out_ptr = np.asarray(out_ptr).astype(np.int64)
    out_dst = np.asarray(out_dst).astype(np.int64)
    if direction == CHILDREN:
        return [[int(c) for c in out_dst[out_ptr[v]:out_ptr[v + 1]]] for v in range(n)]
    lists = [[] for _ in range(n)]
    for u in range(n):
        for c in out_dst[out_ptr[u]:out_ptr[u + 1]]:
            lists[int(c)].append(u)
    return lists


def order_of(candidates, key):
    """distinct ids: key descending as float64 VALUES (both zeros equal), then ascending id; NaN keys last, among themselves by id;
    without a key ascending id"""
    ids = sorted(set(int(c) for c in candidates))
    if key is None:
        return ids

    def sort_key(u):
        x = float(key[u])
        if math.isnan(x):
            return (1, 0.0, u)
        return (0, -x if x != 0.0 else 0.0, u)          # (+inf first: -(+inf) sorts lowest; -0.0 and +0.0 both become +0.0)
    return sorted(ids, key=sort_key)


def top_links(n, out_ptr, out_dst, key, direction, nodes, m, links=None, n_out=None, degree=None, lists=None):
    """-> (links uint32[len(nodes)][m], n_out int32, degree uint32); the arrays given are written like the library writes them
    (entries past n_out untouched).  lists: edge_lists(...) of this graph and direction, when the caller has them already"""
    lists = edge_lists(n, out_ptr, out_dst, direction) if lists is None else lists
    nodes = np.asarray(nodes).astype(np.int64)
    links = np.zeros((len(nodes), m), np.uint32) if links is None else links
    n_out = np.zeros(len(nodes), np.int32) if n_out is None else n_out
    degree = np.zeros(len(nodes), np.uint32) if degree is None else degree
    for i, v in enumerate(nodes):
        row = lists[int(v)] if 0 <= int(v) < n else []
        best = order_of(row, key)[:m]
        links[i, :len(best)] = best
        n_out[i] = len(best)
        degree[i] = min(len(row), 0xFFFFFFFF)
    return links, n_out, degree


def hit_links(n, out_ptr, out_dst, key, direction, docs, n_hits, m, links, n_out, degree, lists=None):
    """docs [n_q][k] node ids, n_hits [n_q] (clamped to 0 .. k); links [n_q][k][m] / n_out [n_q][k] / degree [n_q][k] are written in
    place for the entries j < n_hits[q] only"""
    docs = np.asarray(docs)
    n_q, k = docs.shape
    lists = edge_lists(n, out_ptr, out_dst, direction) if lists is None else lists
    for q in range(n_q):
        nh = min(max(int(n_hits[q]), 0), k)
        if nh:
            lo, no, do = top_links(n, out_ptr, out_dst, key, direction, docs[q, :nh], m, lists=lists)
            for j in range(nh):
                links[q, j, :no[j]] = lo[j, :no[j]]
            n_out[q, :nh] = no
            if degree is not None:
                degree[q, :nh] = do
    return links, n_out, degree
