"""Plain numpy / Python model of ss_hit_proximity, ss_rerank_hits_by_proximity and ss_score_topk_proximity
(include/spaghetti_rank.h): per (query, hit) the smallest body span that holds every query term the doc has at all, the window re-rank
by w_rank * final + w_prox * bonus, and that re-rank applied to scored rows.  No device, no library.  The span is found per start
value: for every present term the smallest value >= the start (a binary search in the term's sorted list), the end the largest of
them: not the way the LDS path of the kernel walks, and not the all-pairs loop of the CPU test's brute force."""
import numpy as np

from tests.passage_model import body_lists

PROXIMITY_DTYPE = np.dtype([("start", "<f4"), ("end", "<f4"), ("n_present", "<u4"), ("n_occ", "<u4"), ("token_mask", "<u8")])
HIT_DTYPE = np.dtype([("doc", "<u4"), ("_pad", "<u4"), ("title", "<f8"), ("body", "<f8"), ("pagerank", "<f8"), ("final", "<f8")])
NAN_BITS = 0x7FF8000000000000


def occurrences(lists, n_terms, n_docs, tokens, d):
    """-> {slot: float32 values ascending, zeros as +0.0}: the occurrences of every DISTINCT term of `tokens` in doc d that has one;
    a term's slot is the index of its first token"""
    out = {}
    for i, t in enumerate(tokens):
        if tokens.index(t) != i or t >= n_terms or d >= n_docs or (t, d) not in lists:
            continue
        v = np.asarray(lists[(t, d)], dtype=np.float32)
        with np.errstate(invalid="ignore"):
            v = v[(v >= 0) & (v < np.inf)]                  # NaN, -100 and +inf are none
        if len(v):
            out[i] = np.sort(np.where(v == 0, np.float32(0.0), v).astype(np.float32))
    return out


def span_entry(occ, tokens):
    """one PROXIMITY_DTYPE entry from a hit's occurrences"""
    e = np.zeros((), dtype=PROXIMITY_DTYPE)
    if not occ:
        return e
    every = np.sort(np.concatenate(list(occ.values())))
    best = None
    for a in np.unique(every):                              # ascending: an equal difference later on does not replace
        ends = []
        for v in occ.values():
            x = int(np.searchsorted(v, a, side="left"))
            if x == len(v):
                break
            ends.append(v[x])
        if len(ends) < len(occ):
            break                                           # a term has no value >= a: nor for any later start
        b = max(ends)
        diff = np.float64(b) - np.float64(a)
        if best is None or diff < best[0]:
            best = (diff, a, b)
    _, a, b = best
    e["start"], e["end"] = a, b
    e["n_present"] = len(occ)
    e["n_occ"] = int(((every >= a) & (every <= b)).sum()) & 0xFFFFFFFF
    e["token_mask"] = sum(1 << i for i, t in enumerate(tokens) if tokens.index(t) in occ)
    return e


def _queries(q_ptr, q_terms):
    qp = np.asarray(q_ptr).astype(np.int64)
    return [[int(t) for t in np.asarray(q_terms)[qp[q]:qp[q + 1]]] for q in range(len(qp) - 1)]


def proximity_ref(body, n_docs, q_ptr, q_terms, hits_doc, n_hits, body_pos=None, fill=0x00):
    """body: (term_ptr, post_doc, post_w); body_pos: (pos_ptr, pos) of the body table or None; hits_doc uint32 [n_q][k].
    -> PROXIMITY_DTYPE [n_q][k]; entries the definition does not write hold the byte `fill`."""
    hits_doc = np.asarray(hits_doc)
    n_q, k = hits_doc.shape
    out = np.frombuffer(bytes([fill]) * (n_q * k * PROXIMITY_DTYPE.itemsize), dtype=PROXIMITY_DTYPE).reshape(n_q, k).copy()
    lists = body_lists(body, body_pos)
    n_terms = len(body[0]) - 1
    for q, tokens in enumerate(_queries(q_ptr, q_terms)):
        for j in range(int(n_hits[q])):
            out[q, j] = span_entry(occurrences(lists, n_terms, n_docs, tokens, int(hits_doc[q, j])), tokens)
    return out


def bonus_of(e, n_distinct_tokens):
    """the header's prox * cover of one entry, every operation a float64 operation of its own"""
    n_present = int(e["n_present"])
    sp = np.float64(e["end"]) - np.float64(e["start"])
    gaps = np.float64(n_present - 1)
    prox = np.float64(0.0) if n_present < 2 else gaps / max(sp, gaps)
    cover = np.float64(n_present) / np.float64(n_distinct_tokens) if n_distinct_tokens else np.float64(0.0)
    return prox * cover


def rerank_ref(body, n_docs, q_ptr, q_terms, hits, n_hits, w_rank, w_prox, first, k, body_pos=None, fill=0x00):
    """hits: HIT_DTYPE [n_q][k_in] -> (hits_out [n_q][k], n_hits_out [n_q], scores_out float64 [n_q][k], prox_out PROXIMITY_DTYPE
    [n_q][k]); entries the definition does not write hold the byte `fill` (n_hits_out is written whole).  n_hits is clamped to
    [0, k_in] as the kernel clamps a device array."""
    hits = np.asarray(hits)
    n_q, k_in = hits.shape
    filled = lambda dt: np.frombuffer(bytes([fill]) * (n_q * k * dt.itemsize), dtype=dt).reshape(n_q, k).copy()   # noqa: E731
    o_hits, o_sc, o_px = filled(hits.dtype), filled(np.dtype("<f8")), filled(PROXIMITY_DTYPE)
    o_n = np.zeros(n_q, np.int32)
    lists = body_lists(body, body_pos)
    n_terms = len(body[0]) - 1
    w_rank, w_prox = np.float64(w_rank), np.float64(w_prox)
    for q, tokens in enumerate(_queries(q_ptr, q_terms)):
        n = min(max(int(n_hits[q]), 0), k_in)
        big_t = len(set(tokens))
        rows = []                                           # (class, minus the score, window index, score bits, entry)
        for j in range(n):
            d = int(hits["doc"][q, j])
            if d >= n_docs:
                rows.append((2, 0.0, j, NAN_BITS, np.zeros((), PROXIMITY_DTYPE)))
                continue
            e = span_entry(occurrences(lists, n_terms, n_docs, tokens, d), tokens)
            with np.errstate(invalid="ignore", over="ignore"):
                score = w_rank * np.float64(hits["final"][q, j]) + w_prox * bonus_of(e, big_t)
            if np.isnan(score):
                rows.append((1, 0.0, j, NAN_BITS, e))
            else:
                rows.append((0, -float(score), j, int(np.float64(score).view(np.uint64)), e))      # (-(-0.0) == 0.0: the zeros tie)
        rows.sort(key=lambda r: (r[0], r[1], r[2]))
        n_out = min(max(n - first, 0), k)
        o_n[q] = n_out
        for r in range(n_out):
            _, _, j, bits, e = rows[first + r]
            o_hits[q, r] = hits[q, j]
            o_sc.view(np.uint64)[q, r] = bits
            o_px[q, r] = e
    return o_hits, o_n, o_sc, o_px


def score_topk_proximity_ref(body, n_docs, q_ptr, q_terms, window_hits, window_n, w_rank, w_prox, first, k, body_pos=None, fill=0x00):
    """ss_score_topk_proximity given the rows ss_score_topk_masked returns at k = k_window (window_hits [n_q][k_window], window_n):
    the re-rank of exactly those rows"""
    return rerank_ref(body, n_docs, q_ptr, q_terms, window_hits, window_n, w_rank, w_prox, first, k, body_pos=body_pos, fill=fill)
