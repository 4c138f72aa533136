"""The numpy restatement of the hybrid-search definitions in include/spaghetti_rank.h (ss_score_docs, ss_fuse_hits, ss_hybrid_topk):
the row of a given doc from the tables directly (a per-token loop in token order, the NaN rule, FinalRank), and the fusion from ranks,
completed rows and Python's sorted on (isnan, -score, doc).  Outputs are written into the arrays given, only where the definitions
write."""
import numpy as np

from tests import vector_model as vm

HIT_DTYPE = np.dtype([("doc", "<u4"), ("_pad", "<u4"), ("title", "<f8"), ("body", "<f8"), ("pagerank", "<f8"), ("final", "<f8")])
FUSED_DTYPE = np.dtype([("score", "<f8"), ("vec_score", "<i4"), ("lex_rank", "<u2"), ("vec_rank", "<u2")])
VEC_HIT_DTYPE = np.dtype([("doc", "<u4"), ("score", "<i4")])
FUSE_RRF, FUSE_WEIGHTED = 0, 1
UNKNOWN = 0xFFFFFFFF
NAN_BITS = np.uint64(0x7FF8000000000000)


def _posting(table, term, doc):
    """the float32 weight of (term, doc), or None"""
    ptr, docs, w = table
    s, e = int(ptr[term]), int(ptr[term + 1])
    i = s + int(np.searchsorted(docs[s:e], doc))
    return w[i] if i < e and int(docs[i]) == doc else None


def doc_row(world, tokens, doc, query_len=None, probs=None):
    """(title, body, pagerank, final) of one doc under one query: world = dict(n_docs, title, body, mt, mb, prior [n_docs][K] | None)"""
    n_terms = len(world["body"][0]) - 1
    T, B = np.float64(0.0), np.float64(0.0)
    any_t = any_b = False
    for t in tokens:                                        # token order; a repeated token is added again
        t = int(t)
        if t == UNKNOWN or t >= n_terms:
            continue
        w = _posting(world["title"], t, doc) if t < len(world["title"][0]) - 1 else None
        if w is not None:
            T, any_t = T + np.float64(w), True
        w = _posting(world["body"], t, doc)
        if w is not None:
            B, any_b = B + np.float64(w), True
    qmag = np.sqrt(np.float64(len(tokens) if query_len is None else query_len))
    mt = np.float64(world["mt"][doc]) if any_t else np.float64(1.0)
    mb = np.float64(world["mb"][doc]) if any_b else np.float64(1.0)
    with np.errstate(all="ignore"):
        body = B / (mb * qmag)
        title = T / (mt * qmag)
        if np.isnan(body):
            body = np.float64(0.0)
        if np.isnan(title):
            title = np.float64(0.0)
        sqd = np.float64(0.0)
        if probs is not None and world.get("prior") is not None:
            for k in range(world["prior"].shape[1]):        # topic order
                sqd = sqd + np.float64(probs[k]) * np.float64(world["prior"][doc, k])
        final = (np.float64(0.33) * sqd + np.float64(0.38) * title + np.float64(0.29) * body) * np.float64(100.0)
    return title, body, sqd, final


def score_docs(world, q_ptr, q_terms, docs, n_in, out, query_len=None, topic_probs=None, clamp=False):
    """out HIT_DTYPE [n_q][k_in]: rows j < n_in[q] written"""
    k_in = docs.shape[1]
    for q in range(docs.shape[0]):
        n = int(n_in[q])
        if clamp:
            n = min(max(n, 0), k_in)
        tokens = q_terms[int(q_ptr[q]):int(q_ptr[q + 1])]
        for j in range(n):
            d = int(docs[q, j])
            row = np.zeros((), HIT_DTYPE)
            row["doc"] = d
            if d < world["n_docs"]:
                t, b, s, f = doc_row(world, tokens, d, None if query_len is None else int(query_len[q]),
                                     None if topic_probs is None else topic_probs[q])
                row["title"], row["body"], row["pagerank"], row["final"] = t, b, s, f
            out[q, j] = row
    return out


def fuse_score(fp, lex_rank, vec_rank, final, vec_score):
    mode, c, w_lex, w_vec = fp
    w_lex, w_vec = np.float64(w_lex), np.float64(w_vec)
    with np.errstate(all="ignore"):
        if mode == FUSE_RRF:
            a = w_lex / np.float64(int(c) + lex_rank) if lex_rank else np.float64(0.0)
            b = w_vec / np.float64(int(c) + vec_rank) if vec_rank else np.float64(0.0)
            return a + b
        return w_lex * np.float64(final) + w_vec * np.float64(int(vec_score))


def fuse(world, vec_table, q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, fp, first, k, hits_out, n_out, fused_out=None, n_union=None,
         query_len=None, topic_probs=None, clamp=False):
    """fp = (mode, rrf_c, w_lex, w_vec); lex HIT_DTYPE [n_q][k_lex], vec VEC_HIT_DTYPE [n_q][k_vec]; vec_table int8 [n_docs][dim]"""
    n_docs = world["n_docs"]
    for q in range(lex.shape[0]):
        nl, nv = int(n_lex[q]), int(n_vec[q])
        if clamp:
            nl, nv = min(max(nl, 0), lex.shape[1]), min(max(nv, 0), vec.shape[1])
        lex_rank, vec_rank = {}, {}
        for j in range(nl):
            d = int(lex["doc"][q, j])
            if d < n_docs:
                lex_rank.setdefault(d, j + 1)               # the first occurrence; ranks are positions
        for j in range(nv):
            d = int(vec["doc"][q, j])
            if d < n_docs:
                vec_rank.setdefault(d, j + 1)
        tokens = q_terms[int(q_ptr[q]):int(q_ptr[q + 1])]
        cands = []
        for d in sorted(set(lex_rank) | set(vec_rank)):
            lr, vr = lex_rank.get(d, 0), vec_rank.get(d, 0)
            if lr:
                row = lex[q, lr - 1].copy()                 # the 40 bytes given
            else:
                row = np.zeros((), HIT_DTYPE)
                row["doc"] = d
                t, b, s, f = doc_row(world, tokens, d, None if query_len is None else int(query_len[q]),
                                     None if topic_probs is None else topic_probs[q])
                row["title"], row["body"], row["pagerank"], row["final"] = t, b, s, f
            if vr:
                vs = int(vec["score"][q, vr - 1])           # trusted, not recomputed
            else:
                vs = int(np.asarray(qvec[q], np.int8).astype(np.int32) @ np.asarray(vec_table[d], np.int8).astype(np.int32))
            score = fuse_score(fp, lr, vr, row["final"], vs)
            cands.append((d, lr, vr, row, vs, score))
        order = sorted(cands, key=lambda c: (1, 0.0, c[0]) if np.isnan(c[5]) else (0, -float(c[5]), c[0]))
        page = order[first:first + k]
        n_out[q] = len(page)
        if n_union is not None:
            n_union[q] = len(cands)
        for r, (d, lr, vr, row, vs, score) in enumerate(page):
            hits_out[q, r] = row
            if fused_out is not None:
                f = np.zeros((), FUSED_DTYPE)
                f["score"] = score
                f["vec_score"], f["lex_rank"], f["vec_rank"] = vs, lr, vr
                fused_out[q, r] = f
                if np.isnan(score):
                    fused_out["score"].view(np.uint64)[q, r] = NAN_BITS
    return hits_out, n_out, fused_out, n_union


def hybrid(world, vec_table, q_ptr, q_terms, qvec, lex, n_lex, k_window, fp, first, k, hits_out, n_out, fused_out=None, n_union=None,
           mask_id=None, masks=None, query_len=None, topic_probs=None):
    """lex / n_lex: the rows of ss_score_topk_masked at k_window (a scoring call, or the oracle); the vector window from vector_model"""
    n_q = lex.shape[0]
    vec = np.zeros((n_q, k_window), VEC_HIT_DTYPE)
    n_vec = np.zeros(n_q, np.int32)
    vm.topk(qvec, vec_table, k_window, vec, n_vec, mask_id, masks)
    return fuse(world, vec_table, q_ptr, q_terms, qvec, lex, n_lex, vec, n_vec, fp, first, k, hits_out, n_out, fused_out, n_union,
                query_len, topic_probs)
