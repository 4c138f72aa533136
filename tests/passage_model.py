"""Plain numpy model of ss_best_passages (include/spaghetti_rank.h): per (query, hit) the window of `width` body positions that
holds most distinct query terms, then most occurrences, then starts earliest.  No device, no library: the occurrences of a hit are
gathered from the body table's position lists, sorted by value, and every distinct value is tried as a window start."""
import numpy as np

PASSAGE_DTYPE = np.dtype([("start", "<f4"), ("last", "<f4"), ("n_distinct", "<u4"), ("n_occ", "<u4"), ("token_mask", "<u8")])


def body_lists(body, body_pos):
    """(term_ptr, post_doc, ...), (pos_ptr, pos) -> {(term, doc): float32 array of the posting's position list}; {} without positions"""
    if body_pos is None:
        return {}
    ptr, doc = np.asarray(body[0]).astype(np.int64), np.asarray(body[1])
    pp, pos = np.asarray(body_pos[0]).astype(np.int64), np.asarray(body_pos[1], dtype=np.float32)
    return {(t, int(doc[x])): pos[pp[x]:pp[x + 1]] for t in range(len(ptr) - 1) for x in range(int(ptr[t]), int(ptr[t + 1]))}


def occurrences(lists, n_terms, n_docs, tokens, d):
    """-> (values float32 ascending with zeros as +0.0, slots): one entry per occurrence of a DISTINCT term of `tokens` in doc d; a
    term's slot is the index of its first token"""
    vals, slots = [], []
    for i, t in enumerate(tokens):
        if tokens.index(t) != i or t >= n_terms or d >= n_docs or (t, d) not in lists:
            continue
        v = lists[(t, d)]
        with np.errstate(invalid="ignore"):
            v = v[v >= 0]                                   # NaN >= 0 and -100 >= 0 are false
        vals.append(np.where(v == 0, np.float32(0.0), v).astype(np.float32))
        slots.append(np.full(len(v), i, dtype=np.int64))
    if not vals:
        return np.zeros(0, np.float32), np.zeros(0, np.int64)
    vals, slots = np.concatenate(vals), np.concatenate(slots)
    order = np.argsort(vals, kind="stable")
    return vals[order], slots[order]


def best_window(vals, slots, tokens, width):
    """one PASSAGE_DTYPE entry from a hit's occurrences"""
    e = np.zeros((), dtype=PASSAGE_DTYPE)
    best = (0, 0)
    v64 = vals.astype(np.float64)
    for p in np.unique(vals):                               # ascending: an equal (n_distinct, n_occ) later on does not replace
        inside = (vals >= p) & (v64 < np.float64(p) + np.float64(width))
        cand = (len(set(slots[inside].tolist())), int(inside.sum()))
        if cand[1] and cand > best:
            best = cand
            e["start"], e["last"] = p, vals[inside].max()
            e["n_distinct"], e["n_occ"] = cand[0], cand[1] & 0xFFFFFFFF
            have = set(slots[inside].tolist())
            e["token_mask"] = sum(1 << i for i, t in enumerate(tokens) if tokens.index(t) in have)
    return e


def passages_ref(body, n_docs, q_ptr, q_terms, hits_doc, n_hits, width, body_pos=None, fill=0x00):
    """body: (term_ptr, post_doc, post_w); body_pos: (pos_ptr, pos) of the body table or None; hits_doc uint32 [n_q][k].
    -> PASSAGE_DTYPE [n_q][k]; entries the definition does not write hold the byte `fill`."""
    hits_doc = np.asarray(hits_doc)
    n_q, k = hits_doc.shape
    out = np.frombuffer(bytes([fill]) * (n_q * k * PASSAGE_DTYPE.itemsize), dtype=PASSAGE_DTYPE).reshape(n_q, k).copy()
    lists = body_lists(body, body_pos)
    n_terms = len(body[0]) - 1
    qp = np.asarray(q_ptr).astype(np.int64)
    for q in range(n_q):
        tokens = [int(t) for t in np.asarray(q_terms)[qp[q]:qp[q + 1]]]
        for j in range(int(n_hits[q])):
            vals, slots = occurrences(lists, n_terms, n_docs, tokens, int(hits_doc[q, j]))
            out[q, j] = best_window(vals, slots, tokens, width)
    return out
