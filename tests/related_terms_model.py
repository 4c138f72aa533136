"""numpy model of "related terms" (include/spaghetti_rank.h: ss_related_terms), built on tests/doc_view_model.top_terms.
No GPU, no library call.
"""
import math

import numpy as np

from tests import doc_view_model as dvm


def sum_in_order(weights):
    """float64 sum of float32 weights, one addend at a time in the order given, starting from 0.0 (NOT np.sum: pairwise summation
    would add in another order, and the order is part of the definition)."""
    s = np.float64(0.0)
    for w in weights:
        s = s + np.float64(np.float32(w))
    return s


def candidate_order(terms, scores):
    """Positions of the candidates in output order: score descending as float64 VALUES (-0.0 == +0.0), then ascending term id;
    NaN last, NaNs among themselves by term id."""
    def key(i):
        x = float(scores[i])
        return (1, 0.0, int(terms[i])) if math.isnan(x) else (0, -x, int(terms[i]))
    return sorted(range(len(terms)), key=key)


def related_ref(rows, n_rows, view, q_ptr, q_terms, m_doc, m):
    """rows [n_q][k_fb] hits (HIT_DTYPE) with n_rows [n_q] of them valid, view = doc_view_model.doc_view of the BODY table
    -> (terms uint32[n_q][m], score float64[n_q][m], n_out int32[n_q]); entries past n_out[q] are zero."""
    q_ptr = np.asarray(q_ptr).astype(np.int64)
    q_terms = np.asarray(q_terms)
    n_q = len(q_ptr) - 1
    terms = np.zeros((n_q, m), dtype=np.uint32)
    score = np.zeros((n_q, m), dtype=np.float64)
    n_out = np.zeros(n_q, dtype=np.int32)
    for q in range(n_q):
        docs = rows["doc"][q, :int(n_rows[q])]
        typed = {int(t) for t in q_terms[q_ptr[q]:q_ptr[q + 1]]}
        t_hit, w_hit, cnt = dvm.top_terms(view, docs, m_doc)
        addends = {}                                     # term -> its weights in rank order (dicts keep insertion order)
        for j in range(len(docs)):
            for i in range(int(cnt[j])):
                t = int(t_hit[j, i])
                if t not in typed:
                    addends.setdefault(t, []).append(w_hit[j, i])
        cand = list(addends)
        sums = [sum_in_order(addends[t]) for t in cand]
        pick = candidate_order(cand, sums)[:m]
        n_out[q] = len(pick)
        terms[q, :len(pick)] = [cand[i] for i in pick]
        score[q, :len(pick)] = [sums[i] for i in pick]  # the sums' bits
    return terms, score, n_out
