"""ss_field_stats and ss_field_histogram in numpy and Python integers, straight from their definitions (include/spaghetti_rank.h): the
match sets of tests/facet_model.py; per query the values of its matches, those equal to SS_NO_FIELD_VALUE set aside as missing; min, max
and a Python-int sum split into sum_lo / sum_hi; the bin of every value by Python's exact integer division or by bisection over the
edges.  Nothing here calls the library or knows how its kernels reduce, divide or search."""
import bisect

import numpy as np

from tests import facet_model as fm

I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
NO_VALUE = I64_MIN               # SS_NO_FIELD_VALUE
MAX_HIST_BINS = 65536            # SS_MAX_HIST_BINS
FIELD_STAT_DTYPE = np.dtype([("min", "<i8"), ("max", "<i8"), ("sum_lo", "<u8"), ("sum_hi", "<i8"), ("count", "<u4"), ("missing", "<u4")])   # ss_field_stat
HIST_TAIL_DTYPE = np.dtype([("below", "<u4"), ("above", "<u4"), ("missing", "<u4"), ("n_match", "<u4")])   # ss_hist_tail


def split_sum(total):
    """a Python integer -> (sum_lo, sum_hi) of its 128-bit two's complement form"""
    t = total % (1 << 128)
    lo, hi = t & (2 ** 64 - 1), t >> 64
    return lo, hi - (1 << 64) if hi >= 1 << 63 else hi


def stat_of(values):
    """int64 values of a query's matches in one field -> one FIELD_STAT_DTYPE entry"""
    v = [int(x) for x in values]
    have = [x for x in v if x != NO_VALUE]
    lo, hi = split_sum(sum(have))
    return (min(have) if have else I64_MAX, max(have) if have else I64_MIN, lo, hi, len(have), len(v) - len(have))


def field_stats(n_docs, title, body, q_ptr, q_terms, fields, stat_fields, masks=None, mask_id=None, req=None, exc=None, ranges=None):
    """-> (stats FIELD_STAT_DTYPE [n_q][len(stat_fields)], n_match uint32 [n_q]) and the match sets (bool [n_q][n_docs]).  Arguments as
    facet_model.facet_counts'; fields: int64 [n_fields][n_docs]."""
    n_match, _, _, sets = fm.facet_counts(n_docs, title, body, q_ptr, q_terms, masks=masks, fields=fields, mask_id=mask_id, req=req, exc=exc,
                                          ranges=ranges)
    n_q = len(q_ptr) - 1
    stats = np.zeros((n_q, len(stat_fields)), dtype=FIELD_STAT_DTYPE)
    for q in range(n_q):
        docs = np.nonzero(sets[q])[0]
        for i, f in enumerate(stat_fields):
            stats[q, i] = stat_of(np.asarray(fields[f], dtype=np.int64)[docs])
    return stats, n_match, sets


def histogram_of(values, n_bins, origin=0, width=1, edges=None):
    """int64 values -> (counts uint32 [n_bins], below, above, missing)"""
    counts = np.zeros(n_bins, dtype=np.uint32)
    below = above = missing = 0
    edges = None if edges is None else [int(e) for e in edges]
    uniq, cnt = np.unique(np.asarray(values, dtype=np.int64), return_counts=True)
    for v, c in zip((int(x) for x in uniq), (int(x) for x in cnt)):
        if v == NO_VALUE:
            missing += c
        elif edges is not None:
            if v < edges[0]:
                below += c
            elif v >= edges[n_bins]:
                above += c
            else:
                counts[bisect.bisect_right(edges, v) - 1] += c
        elif v < origin:
            below += c
        elif (v - origin) // width >= n_bins:
            above += c
        else:
            counts[(v - origin) // width] += c
    return counts, below, above, missing


def field_histogram(n_docs, title, body, q_ptr, q_terms, fields, field, n_bins, origin=0, width=1, edges=None, masks=None, mask_id=None, req=None,
                    exc=None, ranges=None):
    """-> (counts uint32 [n_q][n_bins], tails HIST_TAIL_DTYPE [n_q]) and the match sets"""
    n_match, _, _, sets = fm.facet_counts(n_docs, title, body, q_ptr, q_terms, masks=masks, fields=fields, mask_id=mask_id, req=req, exc=exc,
                                          ranges=ranges)
    n_q = len(q_ptr) - 1
    counts = np.zeros((n_q, n_bins), dtype=np.uint32)
    tails = np.zeros(n_q, dtype=HIST_TAIL_DTYPE)
    col = np.asarray(fields[field], dtype=np.int64)
    for q in range(n_q):
        counts[q], below, above, missing = histogram_of(col[np.nonzero(sets[q])[0]], n_bins, origin, width, edges)
        tails[q] = (below, above, missing, int(n_match[q]))
    return counts, tails, sets
