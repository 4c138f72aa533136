"""The definition of ss_maxsim_topk (include/spaghetti_rank.h) as plain loops over tests/maxsim_model.py's maxsim(q, d): every doc with
a token that the query's mask allows is a candidate, the candidates are ordered by (score descending, doc ascending), and the first k
are written.  Outputs are written into the arrays given, only where the definition writes."""
import numpy as np

from tests.maxsim_model import maxsim

VEC_HIT_DTYPE = np.dtype([("doc", "<u4"), ("score", "<i4")])


def candidates(qt_ptr, qtok, tok_ptr, tok, q, allowed=None):
    """[(doc, score)] of query q in the definition's order; allowed: bool [>= n_docs] or None = every doc"""
    n_docs = len(tok_ptr) - 1
    qrows = np.asarray(qtok)[int(qt_ptr[q]):int(qt_ptr[q + 1])] if qtok is not None else np.zeros((0, np.asarray(tok).shape[1]), np.int8)
    rows = []
    for d in range(n_docs):
        a, b = int(tok_ptr[d]), int(tok_ptr[d + 1])
        if b == a:
            continue                                                        # a doc without tokens is never a candidate
        if allowed is not None and not allowed[d]:
            continue
        rows.append((d, maxsim(qrows, np.asarray(tok)[a:b])))
    rows.sort(key=lambda r: (-r[1], r[0]))
    return rows


def topk(qt_ptr, qtok, tok_ptr, tok, k, hits, n_hits, mask_id=None, masks=None):
    """hits: VEC_HIT_DTYPE [n_q][k], n_hits int32 [n_q]; masks: bool [n_masks][>= n_docs], mask_id int [n_q] or None = all -1"""
    n_q = len(qt_ptr) - 1
    for q in range(n_q):
        allowed = None
        if mask_id is not None and int(mask_id[q]) >= 0:
            allowed = masks[int(mask_id[q])]
        rows = candidates(qt_ptr, qtok, tok_ptr, tok, q, allowed)[:k]
        n_hits[q] = len(rows)
        for r, (d, s) in enumerate(rows):
            hits[q, r] = (d, s)
    return hits, n_hits
