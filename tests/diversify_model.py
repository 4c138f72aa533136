"""The numpy restatement of ss_diversify_hits as include/spaghetti_rank.h defines it: the window's Gram matrix as a float64 matmul of
the int8 rows (exact: every entry is an integer below 2^53, and an int64 matmul has no BLAS), relevance from the query vector or the
window position, and the greedy walk in int64.  Outputs are written into the arrays given, only where the definition writes."""
import numpy as np

NO_SCORE = -(2 ** 31)            # SS_NO_VEC_SCORE
WEIGHT_MAX = 65536               # SS_DIV_WEIGHT_MAX
INFO_DTYPE = np.dtype([("rel", "<i4"), ("sim", "<i4")])   # ss_div_info


def gram(vec, docs):
    """int64 [n][n]: sim(i, j) of the window rows whose docs (all inside the table) are given"""
    rows = np.asarray(vec, np.int8)[np.asarray(docs, np.int64)].astype(np.float64)
    return (rows @ rows.T).astype(np.int64)


def walk(rel, sim, w_rel, w_div, n_choices):
    """the first n_choices choices over rows with relevance rel [m] (int64) and similarities sim [m][m] (int64) ->
    (order [c], pen at the moment of choice [c]; the first entry of pen is NO_SCORE)"""
    m = len(rel)
    rel = np.asarray(rel, np.int64)
    pen = np.zeros(m, np.int64)
    live = np.ones(m, bool)
    order, pens = [], []
    for c in range(min(n_choices, m)):
        value = np.int64(w_rel) * rel - np.int64(w_div) * pen
        value = np.where(live, value, np.iinfo(np.int64).min)
        j = int(np.argmax(value))                 # the first of the largest: the smaller window index
        order.append(j)
        pens.append(int(pen[j]) if c else NO_SCORE)
        live[j] = False
        pen = sim[j].copy() if c == 0 else np.maximum(pen, sim[j])
    return order, pens


def diversify(qvec, vec, hits, n_hits, w_rel, w_div, first, k, hits_out, n_out, info_out=None, clamp=False):
    """qvec None: rel(j) = -j.  hits [n_q][k_in] structured rows; page [first, first + k) of the chosen rows, then the outside rows"""
    v = np.asarray(vec, np.int8)
    n_docs, k_in = v.shape[0], hits.shape[1]
    for q in range(hits.shape[0]):
        n = int(n_hits[q])
        if clamp:
            n = min(max(n, 0), k_in)
        docs = hits["doc"][q, :n].astype(np.int64)
        inside = np.flatnonzero(docs < n_docs)
        outside = np.flatnonzero(docs >= n_docs)
        if qvec is None:
            rel = -inside.astype(np.int64)
        else:
            rel = (v[docs[inside]].astype(np.float64) @ np.asarray(qvec[q], np.int8).astype(np.float64)).astype(np.int64)
        sim = gram(v, docs[inside]) if len(inside) else np.zeros((0, 0), np.int64)
        order, pens = walk(rel, sim, w_rel, w_div, first + k)
        seq = [(int(inside[j]), int(rel[j]), p) for j, p in zip(order, pens)]
        if len(seq) == len(inside):               # (otherwise the page ends inside the chosen rows)
            seq += [(int(j), NO_SCORE, NO_SCORE) for j in outside]
        page = seq[first:first + k]
        n_out[q] = min(max(n - first, 0), k)
        assert len(page) == n_out[q]
        for r, (j, rl, p) in enumerate(page):
            hits_out[q, r] = hits[q, j]
            if info_out is not None:
                info_out[q, r] = (rl, p)
    return hits_out, n_out, info_out
