"""ss_top_groups in numpy, straight from its definition (include/spaghetti_rank.h): the match sets of tests/facet_model.py, per query
np.unique(..., return_counts=True) over the group values of its matches, one np.lexsort by (count descending, value ascending), then
the page.  Nothing here calls the library or knows how its kernels rank or count the groups."""
import numpy as np

from tests import facet_model as fm

NO_GROUP = 0xFFFFFFFF            # SS_NO_GROUP
GROUP_COUNT_DTYPE = np.dtype([("group", "<u4"), ("count", "<u4")])   # ss_group_count


def group_values(group):
    """the distinct values != SS_NO_GROUP of a table, ascending as unsigned 32-bit"""
    v = np.unique(np.asarray(group, dtype=np.uint32))
    return v[v != NO_GROUP]


def order(match, group):
    """bool [n_docs], uint32 [n_docs] -> (the groups with a match in the defined order as GROUP_COUNT_DTYPE, the SS_NO_GROUP matches)"""
    g = np.asarray(group, dtype=np.uint32)[np.nonzero(match)[0]]
    ungrouped = int(np.count_nonzero(g == NO_GROUP))
    v, c = np.unique(g[g != NO_GROUP], return_counts=True)
    o = np.lexsort((v.astype(np.int64), -c.astype(np.int64)))
    rows = np.zeros(len(o), dtype=GROUP_COUNT_DTYPE)
    rows["group"], rows["count"] = v[o], c[o]
    return rows, ungrouped


def top_groups(n_docs, title, body, q_ptr, q_terms, group, first=0, m=10, masks=None, fields=None, mask_id=None, req=None, exc=None,
               ranges=None):
    """-> (rows: list of GROUP_COUNT_DTYPE arrays, one page per query; n_out int32 [n_q]; n_groups, n_ungrouped, n_match uint32 [n_q])
    and the match sets (bool [n_q][n_docs]).  Arguments as facet_model.facet_counts'."""
    n_match, _, _, sets = fm.facet_counts(n_docs, title, body, q_ptr, q_terms, masks=masks, fields=fields, mask_id=mask_id, req=req, exc=exc,
                                          ranges=ranges)
    n_q = len(q_ptr) - 1
    rows, n_groups, n_ungrouped = [], np.zeros(n_q, np.uint32), np.zeros(n_q, np.uint32)
    for q in range(n_q):
        every, n_ungrouped[q] = order(sets[q], group)
        n_groups[q] = len(every)
        rows.append(every[first:first + m])
    n_out = np.array([len(r) for r in rows], dtype=np.int32)
    return rows, n_out, n_groups, n_ungrouped, n_match, sets
