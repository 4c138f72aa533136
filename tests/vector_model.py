"""The numpy restatement of the doc-vector definitions in include/spaghetti_rank.h (ss_vector_topk, ss_hit_vector_scores,
ss_rerank_hits_by_vector): an int32 matmul, np.lexsort on (doc, -score), allow-lists, and the stable re-rank of a window.  Outputs are
written into the arrays given, only where the definitions write."""
import numpy as np

NO_SCORE = -(2 ** 31)            # SS_NO_VEC_SCORE
MAX_DIM = 1024                   # SS_MAX_VEC_DIM


def scores(qvec, vec):
    """int32 [n_q][n_docs]: exact, |score| <= 1024 * 128 * 128 = 2^24"""
    return np.asarray(qvec, np.int8).astype(np.int32) @ np.asarray(vec, np.int8).astype(np.int32).T


def topk(qvec, vec, k, hits, n_hits, mask_id=None, masks=None):
    """hits: a structured array [n_q][k] with fields doc / score, n_hits int32 [n_q]; masks: bool [n_masks][n_docs]"""
    sc = scores(qvec, vec)
    n_docs = sc.shape[1]
    for q in range(sc.shape[0]):
        allowed = np.arange(n_docs)
        if mask_id is not None and mask_id[q] >= 0:
            allowed = np.flatnonzero(masks[mask_id[q]])
        s = sc[q, allowed]
        order = np.lexsort((allowed, -s.astype(np.int64)))[:k]
        n_hits[q] = len(order)
        hits["doc"][q, :len(order)] = allowed[order]
        hits["score"][q, :len(order)] = s[order]
    return hits, n_hits


def hit_scores(qvec, vec, hits, n_hits, out):
    """out int32 [n_q][k_in]: rows j < n_hits[q] written, NO_SCORE for a doc outside the table"""
    qv, v = np.asarray(qvec, np.int8).astype(np.int32), np.asarray(vec, np.int8).astype(np.int32)
    n_docs = v.shape[0]
    for q in range(hits.shape[0]):
        for j in range(int(n_hits[q])):
            d = int(hits["doc"][q, j])
            out[q, j] = int(qv[q] @ v[d]) if d < n_docs else NO_SCORE
    return out


def rerank(qvec, vec, hits, n_hits, first, k, hits_out, n_out, scores_out=None, clamp=False):
    """the window sorted stably by score descending, rows outside the table last in window order; page [first, first + k)"""
    qv, v = np.asarray(qvec, np.int8).astype(np.int32), np.asarray(vec, np.int8).astype(np.int32)
    n_docs, k_in = v.shape[0], hits.shape[1]
    for q in range(hits.shape[0]):
        n = int(n_hits[q])
        if clamp:
            n = min(max(n, 0), k_in)
        docs = hits["doc"][q, :n].astype(np.int64)
        inside = docs < n_docs
        sc = np.array([int(qv[q] @ v[d]) if ok else NO_SCORE for d, ok in zip(docs, inside)], np.int64)
        order = sorted(range(n), key=lambda j: (0, -sc[j], j) if inside[j] else (1, 0, j))[first:first + k]
        n_out[q] = len(order)
        for r, j in enumerate(order):
            hits_out[q, r] = hits[q, j]
            if scores_out is not None:
                scores_out[q, r] = sc[j]
    return hits_out, n_out, scores_out
