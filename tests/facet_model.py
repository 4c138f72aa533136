"""ss_facet_counts in numpy, straight from the sets of its definition (include/spaghetti_rank.h): one boolean array per term from
the CSR tables, OR over a query's usable terms, AND with the allowed set built from ITS definition, count_nonzero.  Nothing here
calls the library or knows how its kernel tiles the docs."""
import numpy as np


def unpack_masks(words, n_docs):
    """uint32 words [n_masks][(n_docs + 31) // 32] -> bool [n_masks][n_docs] (bits at and past n_docs dropped)"""
    words = np.ascontiguousarray(words, dtype="<u4")
    if words.size == 0:
        return np.zeros((0, n_docs), dtype=bool)
    return np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little")[:, :n_docs].astype(bool)


def contains(n_docs, title, body, t):
    """docs with a posting of term t in the title or the body table (ptr, doc), of any weight; none for t >= n_terms"""
    out = np.zeros(n_docs, dtype=bool)
    for ptr, doc in (title, body):
        if 0 <= int(t) < len(ptr) - 1:
            out[np.asarray(doc[int(ptr[t]):int(ptr[t + 1])], dtype=np.int64)] = True
    return out


def matches(fields, clause):
    field, lo, hi = int(clause[0]), int(clause[1]), int(clause[2])
    v = np.asarray(fields[field], dtype=np.int64)
    if lo > hi:
        return np.zeros(v.shape[0], dtype=bool)
    return (v >= np.int64(lo)) & (v <= np.int64(hi))


def allowed_set(n_docs, title, body, masks, fields, mask_id, req, exc, clauses):
    """ss_score_topk_filtered's rule: in the query's mask, contains every required term, no excluded term, matches every clause"""
    a = np.ones(n_docs, dtype=bool) if mask_id is None or mask_id < 0 else masks[mask_id].copy()
    for t in req:
        a &= contains(n_docs, title, body, t)
    for t in exc:
        a &= ~contains(n_docs, title, body, t)
    for c in clauses:
        a &= matches(fields, c)
    return a


def match_set(n_docs, title, body, terms):
    c = np.zeros(n_docs, dtype=bool)
    for t in terms:
        c |= contains(n_docs, title, body, t)
    return c


def _rows(pair, q):
    if pair is None:
        return []
    ptr, items = pair
    return list(items[int(ptr[q]):int(ptr[q + 1])])


def facet_counts(n_docs, title, body, q_ptr, q_terms, masks=None, fields=None, mask_id=None, req=None, exc=None, ranges=None, buckets=()):
    """masks: bool [n_masks][n_docs]; fields: int64 [n_fields][n_docs]; req / exc: (ptr, terms) or None; ranges: (ptr, list of
    (field, lo, hi)) or None; buckets: list of (field, lo, hi) -> (n_match [n_q], mask_counts [n_q][n_masks], bucket_counts
    [n_q][n_buckets]) as uint32, and the match sets themselves (bool [n_q][n_docs])."""
    n_q = len(q_ptr) - 1
    masks = np.zeros((0, n_docs), dtype=bool) if masks is None else np.asarray(masks, dtype=bool)
    n_match = np.zeros(n_q, dtype=np.uint32)
    mask_counts = np.zeros((n_q, masks.shape[0]), dtype=np.uint32)
    bucket_counts = np.zeros((n_q, len(buckets)), dtype=np.uint32)
    sets = np.zeros((n_q, n_docs), dtype=bool)
    for q in range(n_q):
        m = match_set(n_docs, title, body, q_terms[int(q_ptr[q]):int(q_ptr[q + 1])])
        m &= allowed_set(n_docs, title, body, masks, fields, None if mask_id is None else int(mask_id[q]), _rows(req, q), _rows(exc, q),
                         _rows(ranges, q))
        sets[q] = m
        n_match[q] = np.count_nonzero(m)
        for i in range(masks.shape[0]):
            mask_counts[q, i] = np.count_nonzero(m & masks[i])
        for b, bucket in enumerate(buckets):
            bucket_counts[q, b] = np.count_nonzero(m & matches(fields, bucket))
    return n_match, mask_counts, bucket_counts, sets
