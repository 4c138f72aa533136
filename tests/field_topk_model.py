"""ss_field_topk in numpy, straight from its definition (include/spaghetti_rank.h): the match sets of tests/facet_model.py, one
np.lexsort per query by (key, doc) with key = value for ascending and ~value for descending (bitwise NOT reverses signed order without
overflow at INT64_MIN), then the page.  Nothing here calls the library or knows how its kernels cut the docs."""
import numpy as np

from tests import facet_model as fm


def order(match, values, descending):
    """bool [n_docs], int64 [n_docs] -> the matching docs in the defined order (int64 doc ids)"""
    doc = np.nonzero(match)[0]
    v = np.asarray(values, dtype=np.int64)[doc]
    key = ~v if descending else v
    return doc[np.lexsort((doc, key))]


def field_topk(n_docs, title, body, q_ptr, q_terms, fields, field, descending=False, first=0, k=10, masks=None, mask_id=None, req=None,
               exc=None, ranges=None):
    """-> (docs: list of uint32 arrays, one page per query; values: list of int64 arrays; n_out int32 [n_q]; n_match uint32 [n_q]) and
    the match sets (bool [n_q][n_docs]).  Arguments as facet_model.facet_counts'."""
    n_match, _, _, sets = fm.facet_counts(n_docs, title, body, q_ptr, q_terms, masks=masks, fields=fields, mask_id=mask_id, req=req, exc=exc,
                                          ranges=ranges)
    col = np.asarray(fields[field], dtype=np.int64)
    docs, values = [], []
    for q in range(len(q_ptr) - 1):
        page = order(sets[q], col, descending)[first:first + k]
        docs.append(page.astype(np.uint32))
        values.append(col[page])
    n_out = np.array([len(d) for d in docs], dtype=np.int32)
    return docs, values, n_out, n_match, sets
