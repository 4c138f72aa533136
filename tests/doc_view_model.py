"""numpy model of the doc-major view of an inverted table, of a doc's heaviest terms and of "similar pages"
(include/spaghetti_rank.h: ss_index_build_doc_view, ss_index_doc_top_terms, ss_similar_topk).  No GPU, no library call.
"""
import math

import numpy as np


def doc_view(term_ptr, post_doc, post_w, n_docs):
    """-> (doc_ptr uint64[n_docs+1], doc_term uint32[P], doc_w float32[P]): row d = the terms with a posting of d, ascending term id
    (term lists are ascending by doc, so a stable sort of the postings by doc keeps the term order inside a row)."""
    ptr = np.asarray(term_ptr).astype(np.int64)
    doc = np.asarray(post_doc).astype(np.int64)
    w = np.asarray(post_w, dtype=np.float32)
    term = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    order = np.argsort(doc, kind="stable")
    doc_ptr = np.concatenate([[0], np.cumsum(np.bincount(doc, minlength=int(n_docs)))]).astype(np.uint64)
    return doc_ptr, term[order].astype(np.uint32), w[order]


def row_order(terms, w):
    """Positions of a row's entries in the order of ss_index_doc_top_terms: weight descending as float32 VALUES (-0.0 == +0.0),
    then ascending term id; NaN last, NaNs among themselves by term id."""
    def key(i):
        x = float(w[i])
        return (1, 0.0, int(terms[i])) if math.isnan(x) else (0, -x, int(terms[i]))      # (-(-0.0) == -(0.0): the term decides)
    return sorted(range(len(terms)), key=key)


def top_terms(view, docs, m):
    """-> (terms uint32[n][m], w float32[n][m], n_out int32[n]); entries past n_out[i] are zero."""
    doc_ptr, doc_term, doc_w = view
    docs = np.asarray(docs).astype(np.int64)
    terms = np.zeros((len(docs), m), dtype=np.uint32)
    w = np.zeros((len(docs), m), dtype=np.float32)
    n_out = np.zeros(len(docs), dtype=np.int32)
    for i, d in enumerate(docs):
        b, e = int(doc_ptr[d]), int(doc_ptr[d + 1])
        pick = [b + j for j in row_order(doc_term[b:e], doc_w[b:e])[:m]]
        n_out[i] = len(pick)
        terms[i, :len(pick)] = doc_term[pick]
        w[i, :len(pick)] = doc_w[pick]                   # the stored bits (a -0.0 stays -0.0)
    return terms, w, n_out


def queries_of(terms, n_out):
    """top_terms rows -> (q_ptr uint32[n+1], q_terms uint32)."""
    q_ptr = np.concatenate([[0], np.cumsum(n_out)]).astype(np.uint32)
    q_terms = np.concatenate([terms[i, :n_out[i]] for i in range(len(n_out))] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return q_ptr, q_terms


def drop_seed(rows, n_rows, seeds, k):
    """rows [n][k+1] hits -> [n][k]: every row without the hit whose doc is its seed, cut to k, zero behind the last hit."""
    out = np.zeros((len(seeds), k), dtype=rows.dtype)
    n_out = np.zeros(len(seeds), dtype=np.int32)
    for q, seed in enumerate(seeds):
        r = rows[q, :int(n_rows[q])]
        r = r[r["doc"] != np.uint32(seed)][:k]
        out[q, :len(r)] = r
        n_out[q] = len(r)
    return out, n_out


def similar_ref(oracle, n_docs, title, body, mag_t, mag_b, seeds, k, m, prior=None, topic_probs=None, mask_id=None, allowed=None):
    """ss_similar_topk from the model and the CPU oracle: the seeds' top_terms rows in the body view as queries, scored at k + 1
    (under allow-lists: tests/test_gpu_doc_masks.masked_ref over `allowed` bool [n_masks][n_docs]), the seed dropped, cut to k."""
    terms, _, cnt = top_terms(doc_view(*body, n_docs), seeds, m)
    q_ptr, q_terms = queries_of(terms, cnt)
    if mask_id is not None:
        from tests.test_gpu_doc_masks import masked_ref
        rows, n_rows = masked_ref(oracle, n_docs, title, body, mag_t, mag_b, q_ptr, q_terms, mask_id, allowed, k + 1, prior=prior,
                                  topic_probs=topic_probs)
    else:
        kw = {} if prior is None else {"prior": prior, "topic_probs": topic_probs}
        rows, n_rows = oracle.score_topk_batch(n_docs, title, body, mag_t, mag_b, q_ptr, q_terms, k + 1, **kw)
    return drop_seed(rows, n_rows, seeds, k)
