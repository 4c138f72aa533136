"""The doc-field definitions of include/spaghetti_rank.h restated in numpy / plain Python: the words of an allow-list built from range
clauses (ss_doc_field_masks, and the set ss_score_topk_filtered allows), the stable sort of a window by a field with its page
(ss_sort_hits_by_field) and the gather (ss_hit_fields).  Written from the header text, not from the kernels.

values: int64 [n_fields][n_docs].  A clause is (field, lo, hi) and matches doc d iff lo <= values[field][d] <= hi."""
import numpy as np

NO_VALUE = -(2 ** 63)            # SS_NO_FIELD_VALUE
MAX_FIELDS = 4                   # SS_MAX_DOC_FIELDS
MAX_CLAUSES = 4                  # SS_MAX_RANGE_CLAUSES


def matches(values, n_docs, clauses):
    """bool [n_docs]: the docs every clause matches (all of them without a clause)"""
    ok = np.ones(n_docs, dtype=bool)
    for f, lo, hi in clauses:
        col = np.asarray(values[f], dtype=np.int64)
        ok &= (col >= np.int64(lo)) & (col <= np.int64(hi))
    return ok


def pack_bits(bits, n_docs):
    """bool [n_docs] -> uint32 [(n_docs + 31) // 32]: bit (d & 31) of word d >> 5 = doc d; bits at and past n_docs are 0"""
    n_words = (n_docs + 31) // 32
    padded = np.zeros(n_words * 32, dtype=bool)
    padded[:n_docs] = bits[:n_docs]
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def set_words(values, n_docs, sets, mask_id=None, masks=None):
    """uint32 [n_sets][(n_docs + 31) // 32]: set i = registered mask mask_id[i] (bool [n_masks][n_docs]; -1 / None: every doc) AND
    every clause of sets[i]"""
    out = np.zeros((len(sets), (n_docs + 31) // 32), dtype=np.uint32)
    for i, clauses in enumerate(sets):
        m = -1 if mask_id is None else int(mask_id[i])
        base = np.ones(n_docs, dtype=bool) if m < 0 else np.asarray(masks[m], dtype=bool)
        out[i] = pack_bits(base & matches(values, n_docs, clauses), n_docs)
    return out


def _window(n_hits, q, k_in, clamp):
    n = int(n_hits[q])
    if clamp:
        n = min(max(n, 0), k_in)
    assert 0 <= n <= k_in
    return n


def sort_page(hits, n_hits, values, n_docs, field, descending, first, k, out_hits, out_n, out_vals=None, clamp=False):
    """Writes page [first, first + k) of every sorted window into the out arrays (entries past the page untouched) and returns them."""
    n_q, k_in = hits.shape
    for q in range(n_q):
        n = _window(n_hits, q, k_in, clamp)
        inside, outside = [], []
        for j in range(n):
            d = int(hits["doc"][q, j])
            if d < n_docs:
                inside.append((int(values[field][d]), j))
            else:
                outside.append(j)
        inside.sort(key=lambda t: (-t[0], t[1]) if descending else (t[0], t[1]))      # stable: ties in window order
        order = [(j, v) for v, j in inside] + [(j, NO_VALUE) for j in outside]           # rows outside the table last, in window order
        cnt = min(max(n - first, 0), k)
        out_n[q] = cnt
        for r in range(cnt):
            j, v = order[first + r]
            out_hits[q, r] = hits[q, j]
            if out_vals is not None:
                out_vals[q, r] = v
    return out_hits, out_n, out_vals


def gather(hits, n_hits, values, n_docs, out, clamp=False):
    """out [n_q][k_in][n_fields]: rows j < n_hits[q] written, NO_VALUE in every field for a doc outside the table"""
    n_q, k_in = hits.shape
    for q in range(n_q):
        for j in range(_window(n_hits, q, k_in, clamp)):
            d = int(hits["doc"][q, j])
            out[q, j, :] = [int(values[f][d]) for f in range(len(values))] if d < n_docs else NO_VALUE
    return out
