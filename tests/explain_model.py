"""Plain numpy model of ss_explain_hits (include/spaghetti_rank.h): per (query, hit, token) the stored weight bits of the
(term, doc) posting in the title and in the body table, the "posting exists" flags and the smallest body position >= 0.
No device, no library: dict lookups per (term, doc) and Python comparisons on float32 values."""
import numpy as np

TERM_MATCH_DTYPE = np.dtype([("title_w", "<f4"), ("body_w", "<f4"), ("flags", "<u4"), ("body_pos", "<f4")])
HAS_TITLE, HAS_BODY, HAS_POS = 1, 2, 4


def posting_index(table):
    """(term_ptr, post_doc, post_w) -> {(term, doc): position in post_doc / post_w}"""
    ptr, doc = np.asarray(table[0]).astype(np.int64), np.asarray(table[1])
    return {(t, int(doc[x])): x for t in range(len(ptr) - 1) for x in range(int(ptr[t]), int(ptr[t + 1]))}


def earliest_position(values):
    """the smallest v >= 0 of a position list as a float32 value, None if there is none.  NaN >= 0 is false, as is -100 >= 0; the list
    need not be sorted; a smallest value of zero is +0.0 whichever zeros the list holds."""
    best = None
    for v in np.asarray(values, dtype=np.float32):
        if v >= 0 and (best is None or v < best):
            best = v
    if best is None:
        return None
    return np.float32(0.0) if best == 0 else np.float32(best)


def explain_ref(title, body, n_docs, q_ptr, q_terms, hits_doc, n_hits, t_stride, body_pos=None, fill=0x00):
    """title / body: (term_ptr, post_doc, post_w); body_pos: (pos_ptr, pos) of the body table or None; hits_doc uint32 [n_q][k].
    -> TERM_MATCH_DTYPE [n_q][k][t_stride]; entries the definition does not write hold the byte `fill`."""
    hits_doc = np.asarray(hits_doc)
    n_q, k = hits_doc.shape
    out = np.frombuffer(bytes([fill]) * (n_q * k * t_stride * TERM_MATCH_DTYPE.itemsize), dtype=TERM_MATCH_DTYPE).reshape(n_q, k, t_stride).copy()
    t_idx, b_idx = posting_index(title), posting_index(body)
    t_w, b_w = np.asarray(title[2], dtype=np.float32), np.asarray(body[2], dtype=np.float32)
    t_terms, b_terms = len(title[0]) - 1, len(body[0]) - 1
    qp = np.asarray(q_ptr).astype(np.int64)
    for q in range(n_q):
        toks = [int(t) for t in np.asarray(q_terms)[qp[q]:qp[q + 1]]]
        assert len(toks) <= t_stride
        for j in range(int(n_hits[q])):
            d = int(hits_doc[q, j])
            for i, t in enumerate(toks):
                e = np.zeros((), dtype=TERM_MATCH_DTYPE)
                if d < n_docs:
                    if t < t_terms and (t, d) in t_idx:
                        e["title_w"] = t_w[t_idx[(t, d)]]
                        e["flags"] |= HAS_TITLE
                    if t < b_terms and (t, d) in b_idx:
                        x = b_idx[(t, d)]
                        e["body_w"] = b_w[x]
                        e["flags"] |= HAS_BODY
                        if body_pos is not None:
                            first = earliest_position(np.asarray(body_pos[1])[int(body_pos[0][x]):int(body_pos[0][x + 1])])
                            if first is not None:
                                e["body_pos"] = first
                                e["flags"] |= HAS_POS
                out[q, j, i] = e
    return out
