"""The definition of ss_collapse_hits (include/spaghetti_rank.h) as a plain sequential walk: "keep a hit unless its site already has
g".  No sorting, no ranks: one pass over the window with a counter per group, a second pass for the sizes."""
from __future__ import annotations

import numpy as np

NO_GROUP = 0xFFFFFFFF

HIT_DTYPE = np.dtype([("doc", "<u4"), ("_pad", "<u4"), ("title", "<f8"), ("body", "<f8"), ("pagerank", "<f8"), ("final", "<f8")])


def row_groups(docs, group):
    """The group of every window row as a hashable: ("g", value) for a row of the table, ("own", j) for a row of its own."""
    out = []
    for j, d in enumerate(docs):
        d = int(d)
        if d < len(group) and int(group[d]) != NO_GROUP:
            out.append(("g", int(group[d])))
        else:
            out.append(("own", j))
    return out


def collapse_row(docs, group, g):
    """-> (kept window indices in window order, same[j] for every window row j)."""
    grp = row_groups(docs, group)
    seen = {}
    kept = []
    for j, key in enumerate(grp):
        have = seen.get(key, 0)
        if have < g:
            kept.append(j)
        seen[key] = have + 1
    same = [seen[key] for key in grp]
    return kept, same


def collapse(hits, n_hits, group, g, first, k, hits_out, n_hits_out, same_out=None, n_kept_out=None, clamp=False):
    """Writes the outputs the way the call does (entries past n_hits_out[q] untouched) into the arrays given, and returns them.
    hits [n_q][k_in] HIT_DTYPE; clamp: n_hits outside [0, k_in] is clamped (device n_hits), else it is an error."""
    n_q, k_in = hits.shape
    for q in range(n_q):
        n = int(n_hits[q])
        if n < 0 or n > k_in:
            if not clamp:
                raise ValueError("n_hits outside [0, k_in]")
            n = min(max(n, 0), k_in)
        kept, same = collapse_row(hits["doc"][q, :n], group, g)
        page = kept[first:first + k]
        for r, j in enumerate(page):
            hits_out[q, r] = hits[q, j]
            if same_out is not None:
                same_out[q, r] = same[j]
        n_hits_out[q] = len(page)
        if n_kept_out is not None:
            n_kept_out[q] = len(kept)
    return hits_out, n_hits_out, same_out, n_kept_out
